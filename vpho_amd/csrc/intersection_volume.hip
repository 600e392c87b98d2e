// Hand-object intersection volume (--eval_volume).  Per (hand, object pose) pair, in the object's model frame:
//   hand mesh: q_v = R^T (v - t) (fp64, pen_model_frame: the bits of penetration_kernel) with one closed face list shared by all pairs;
//   object solid: the fp32 centres of the cells of a lattice of pitch h over the object's bbox that are inside the object (built once
//     per object by the single-pose penetration kernel at identity pose, vpho_amd/ops.py);
//   inside_hand(c): the z-ray parity rule of penetration.hip against the posed hand mesh in its own hash frame -- the point-independent
//     terms of every face, which penetration.hip gets from the host once per object (physics_eval.mesh_tables), are built HERE per
//     pair (the hand changes with every image), in that function's order of operations; the library is built with -ffp-contract=off,
//     so the 19 fields have the host function's bits and the flags are those of the reference test on the posed mesh;
//   n_cells = number of solid centres inside the hand (integer adds: exact in any order), IV = ((h h) h) n_cells.
// hand_mesh_setup_kernel, one workgroup per pair: pass 1 over the face corners gives the mesh's bbox (min / max: exact, order-free) --
// over the corners, not over all vertices, as the reference takes it from triangles.reshape(-1, 3) --, pass 2 recomputes the three corners
// of every face (the same function on the same inputs: the same bits; V is free, so nothing per vertex is kept) and writes its record.
// solid_inside_count_kernel, grid (point chunks, pairs), one thread per centre: the [0, 512]^3 cull comes first, and a workgroup none of
// whose centres has a hash cell leaves before any record is read (k runs fastest along a lattice column, so a chunk is a compact piece of
// the object: most of them miss the hand's bbox altogether).  The others stream the pair's records through LDS in tiles of 256 (19 fp64
// each: 38 KB; 1 552 x 19 x 8 B = 236 KB do not fit at once) and give every record to pen_parity_step (cell rectangle first).
// gfx950, -O3: no scratch in any of the three kernels (tests/test_volume_cpu.py reads the compiler's report).
#include "common.h"
#include "../../include/vpho_hip.h"
#include "penetration_common.h"

namespace {

constexpr int VOL_THREADS = 256;
constexpr int VOL_TILE = 256;                          // records staged per LDS tile: 256 x 19 doubles = 38 KB
constexpr int VS = VPHO_VOL_TRI_STRIDE;
static_assert(VS == R_CY1 + 1, "the volume records are fields 0 .. 18 of the penetration record");

struct VolArgs {
    vpho_obj_solids s;
    int n_obj;
    const int* faces;            // (F, 3)
    int F;
    const float* verts;          // (n, V, 3)
    const double* rt;            // (n, 3, 4)
    const int* obj_id;           // (n,)
    int n, V;
    double cell_volume;          // (h * h) * h
    double* out;                 // (n, 2)
    unsigned char* flags;        // (n, max_pts) or NULL
    double* rec;                 // workspace: (n, F, VS)
    double* box;                 // workspace: (n, 6) scale | translate
    int* counter;                // workspace: (n, 2) n_cells | bad
};

__global__ __launch_bounds__(VOL_THREADS) void hand_mesh_setup_kernel(const VolArgs a) {
    __shared__ double s_lo[3][VOL_THREADS], s_hi[3][VOL_THREADS];
    __shared__ double s_box[6];
    const int pair = blockIdx.x, tid = threadIdx.x;
    const double* R = a.rt + (long long)pair * 12;
    const float* verts = a.verts + (long long)pair * a.V * 3;
    // ---- pass 1: bbox of the face corners
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    int bad = 0;
    for (int f = tid; f < a.F; f += VOL_THREADS) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int vi = a.faces[3 * f + c];
            if (vi < 0 || vi >= a.V) { bad = 1; continue; }
            double p[3];
            pen_model_frame(R, verts + (long long)vi * 3, p[0], p[1], p[2]);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                bad |= !(fabs(p[k]) <= 1.79769313486231570815e+308);          // NaN or infinite
                lo[k] = fmin(lo[k], p[k]);
                hi[k] = fmax(hi[k], p[k]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) { s_lo[k][tid] = lo[k]; s_hi[k][tid] = hi[k]; }
    bad = __syncthreads_or(bad);
    for (int h = VOL_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                s_lo[k][tid] = fmin(s_lo[k][tid], s_lo[k][tid + h]);
                s_hi[k][tid] = fmax(s_hi[k][tid], s_hi[k][tid + h]);
            }
        }
        __syncthreads();
    }
    if (tid < 3) {
        // MeshIntersector.__init__: scale = (resolution - 1) / (bbox_max - bbox_min), translate = 0.5 - scale * bbox_min
        const double sc = (double)(VPHO_PEN_RESOLUTION - 1) / (s_hi[tid][0] - s_lo[tid][0]);
        const double tr = 0.5 - sc * s_lo[tid][0];
        s_box[tid] = sc; s_box[3 + tid] = tr;
        a.box[(long long)pair * 6 + tid] = sc;
        a.box[(long long)pair * 6 + 3 + tid] = tr;
    }
    if (tid == 0) { a.counter[2 * pair] = 0; a.counter[2 * pair + 1] = bad; }
    __syncthreads();
    if (bad) return;                                   // the pair gets NaN (volume_finish_kernel); its records are never read
    // ---- pass 2: the 19 parity fields of every face, physics_eval.mesh_tables' order of operations
    for (int f = tid; f < a.F; f += VOL_THREADS) {
        double t[3][3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double px, py, pz;
            pen_model_frame(R, verts + (long long)a.faces[3 * f + c] * 3, px, py, pz);
            pen_hash_frame(s_box, s_box + 3, px, py, pz, t[c][0], t[c][1], t[c][2]);
        }
        pen_face_record(t, a.rec + ((long long)pair * a.F + f) * VS);
    }
}

__global__ __launch_bounds__(VOL_THREADS) void solid_inside_count_kernel(const VolArgs a) {
    __shared__ double tile[VOL_TILE * VS];
    const int pair = blockIdx.y, tid = threadIdx.x;
    const int o = a.obj_id[pair];
    if (!(o >= 0 && o < a.n_obj)) return;              // the whole workgroup; volume_finish_kernel writes NaN, the host zeroes the flags
    if (a.counter[2 * pair + 1]) return;
    const int pb = a.s.pt_offset[o], np = a.s.pt_offset[o + 1] - pb;
    if ((long long)blockIdx.x * VOL_THREADS >= np) return;
    const int pi = blockIdx.x * VOL_THREADS + tid;
    const bool live = pi < np;
    double qx = -1.0, qy = -1.0, qz = -1.0;
    if (live) {
        const float* c = a.s.pts + ((long long)pb + pi) * 3;
        const double* box = a.box + (long long)pair * 6;
        pen_hash_frame(box, box + 3, (double)c[0], (double)c[1], (double)c[2], qx, qy, qz);
    }
    double cx, cy;
    const bool has_cell = pen_cell(qx, qy, qz, cx, cy) && live;
    if (!__syncthreads_or(has_cell ? 1 : 0)) return;   // no centre of this chunk inside the hand's [0, 512]^3: no record is read
    unsigned par0 = 0, par1 = 0;
    const double* rec = a.rec + (long long)pair * a.F * VS;
    for (int t0 = 0; t0 < a.F; t0 += VOL_TILE) {
        const int cnt = min(VOL_TILE, a.F - t0);
        __syncthreads();
        const double* src = rec + (long long)t0 * VS;
        for (int i = tid; i < cnt * VS; i += VOL_THREADS) tile[i] = src[i];
        __syncthreads();
        if (!has_cell) continue;
        for (int k = 0; k < cnt; ++k) pen_parity_step(tile + k * VS, qx, qy, qz, cx, cy, par0, par1);
    }
    const bool ins = par0 && par1;
    if (a.flags && live && ins) a.flags[(long long)pair * a.s.max_pts + pi] = 1;
    const int total = __syncthreads_count(ins ? 1 : 0);
    if (tid == 0 && total) atomicAdd(a.counter + 2 * pair, total);
}

// one thread per pair: n_cells as fp64 and IV = cell_volume * n_cells; NaN for a bad object id or a bad hand mesh
__global__ __launch_bounds__(256) void volume_finish_kernel(const VolArgs a) {
    const int pair = blockIdx.x * 256 + threadIdx.x;
    if (pair >= a.n) return;
    const int o = a.obj_id[pair];
    const bool bad = !(o >= 0 && o < a.n_obj) || a.counter[2 * pair + 1];
    const double cells = (double)a.counter[2 * pair];
    a.out[2 * (long long)pair] = bad ? NAN : cells;
    a.out[2 * (long long)pair + 1] = bad ? NAN : a.cell_volume * cells;
}

long long workspace_bytes(long long n, long long F) { return 8 * (n * F * VS + n * 6) + 8 * n; }

}  // namespace

extern "C" long long vpho_hand_obj_intersection_workspace_bytes(int n, int F) {
    if (n < 0 || F <= 0) return -1;
    return workspace_bytes(n, F);
}

extern "C" int vpho_hand_obj_intersection_f64(const vpho_obj_mesh_tables* t, const vpho_obj_solids* solids, const int* faces, int F, const float* verts,
                                              int n, int V, const double* obj_rt, const int* obj_id, double pitch, double* out, unsigned char* flags,
                                              void* workspace, long long workspace_bytes_given, void* stream) {
    VPHO_REQUIRE(t && t->n_obj > 0, "vpho_hand_obj_intersection_f64: bad mesh tables");
    VPHO_REQUIRE(solids && solids->pts && solids->pt_offset && solids->n_obj == t->n_obj && solids->max_pts >= 0,
                 "vpho_hand_obj_intersection_f64: bad solid tables (they must cover the %d objects of the mesh tables)", t->n_obj);
    VPHO_REQUIRE(F > 0, "vpho_hand_obj_intersection_f64: a hand mesh without faces (F=%d)", F);
    VPHO_REQUIRE(pitch > 0.0, "vpho_hand_obj_intersection_f64: the voxel pitch must be positive (%g)", pitch);
    VPHO_REQUIRE(n >= 0 && V > 0 && n <= 65535, "vpho_hand_obj_intersection_f64: bad shape (n=%d, V=%d)", n, V);
    if (n == 0) return 0;
    VPHO_REQUIRE(faces && verts && obj_rt && obj_id && out, "vpho_hand_obj_intersection_f64: bad argument");
    const long long need = workspace_bytes(n, F);
    VPHO_REQUIRE(workspace && workspace_bytes_given >= need, "vpho_hand_obj_intersection_f64: workspace of %lld bytes, %lld needed", workspace_bytes_given, need);
    hipStream_t s = (hipStream_t)stream;
    VolArgs a;
    a.s = *solids; a.n_obj = t->n_obj; a.faces = faces; a.F = F; a.verts = verts; a.rt = obj_rt; a.obj_id = obj_id; a.n = n; a.V = V;
    a.cell_volume = (pitch * pitch) * pitch;
    a.out = out; a.flags = flags;
    a.rec = (double*)workspace;
    a.box = a.rec + (long long)n * F * VS;
    a.counter = (int*)(a.box + (long long)n * 6);
    if (flags && solids->max_pts > 0) VPHO_HIP(hipMemsetAsync(flags, 0, (size_t)n * solids->max_pts, s));
    hipLaunchKernelGGL(hand_mesh_setup_kernel, dim3(n), dim3(VOL_THREADS), 0, s, a);
    int rc = vpho::check_launch("hand_mesh_setup_kernel");
    const int chunks = (solids->max_pts + VOL_THREADS - 1) / VOL_THREADS;
    if (!rc && chunks > 0) {
        hipLaunchKernelGGL(solid_inside_count_kernel, dim3(chunks, n), dim3(VOL_THREADS), 0, s, a);
        rc = vpho::check_launch("solid_inside_count_kernel");
    }
    if (!rc) {
        hipLaunchKernelGGL(volume_finish_kernel, dim3((n + 255) / 256), dim3(256), 0, s, a);
        rc = vpho::check_launch("volume_finish_kernel");
    }
    return rc;
}
