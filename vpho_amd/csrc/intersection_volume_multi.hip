// Hand-object intersection volume of EVERY sampled hypothesis (--eval_best with --eval_volume): what
// intersection_volume.hip gives for the n x S (hand hypothesis s, object hypothesis s) pairs, bit for bit, without its visit of every
// face by every solid centre and without its [pairs][F][19] fp64 records in memory.
// The object's solid keeps lattice order with k (z) fastest (physics_eval.solid_lattice, ops.build_solids), so the centres of one
// lattice column are a contiguous run of pts with the same fp32 x and y (vpho_obj_solid_columns: the run starts).  The hand's hash frame
// is a per-axis scale + translate, so all centres of a column have the same bits of q_x, q_y and, where they have a cell at all, of the
// cell (c_x, c_y).  The cell test, the strict containment and the plane depth of pen_parity_step depend on (q_x, q_y) and the face only:
// pen_parity_xy runs once per (column, face), and only on a hit -- a handful of faces per column -- pen_parity_z runs per centre, on the
// operands it has in the per-pair kernel.  The parities are XOR counts, so the order of the faces and of the centres is free.
// column_walk_kernel, one workgroup per pair:
//   1. bbox of the posed face corners (min / max: exact, order-free), as hand_mesh_setup_kernel pass 1 -> the hash frame; a non-finite
//      corner or a face index outside [0, V) makes the pair NaN before any record is built;
//   2. the object's columns in windows of 256, one per thread: a column whose (q_x, q_y) has no hash cell leaves at once; the others are
//      pushed, in pieces of 64 centres, onto a work list in LDS.  Whenever the list holds 256 pieces (and once more at the end) the
//      workgroup walks them: the face records are built tile by tile IN LDS (256 x 19 fp64 = 38 KB, the arithmetic of
//      hand_mesh_setup_kernel pass 2: the same function on the same inputs) and every thread takes its piece through the tile -- all
//      lanes read the same record (LDS broadcast).  The two parities of a piece's centres are two 64-bit masks in registers.
//      Which thread gets which piece depends on the order of the pushes (an LDS counter); every centre has exactly one owner and the only
//      reduction is an integer add, so the outputs do not depend on it.
// volume_table_kernel, one thread per image: one | best | mean over S (integer sum, one division, one product; NaN written explicitly).
// No workspace.  gfx950, -O3: no scratch, no spills (tests/test_volume_multi_cpu.py reads the compiler's report).
#include "common.h"
#include "../../include/vpho_hip.h"
#include "penetration_common.h"

namespace {

constexpr int VM_THREADS = 256;
constexpr int VM_TILE = 256;                           // records per LDS tile, one built per thread
constexpr int VM_PIECE = 64;                           // centres per work item: one bit each in two 64-bit masks
constexpr int VS = VPHO_VOL_TRI_STRIDE;
static_assert(VS == R_CY1 + 1, "the volume records are fields 0 .. 18 of the penetration record");
static_assert(VM_TILE == VM_THREADS && VM_TILE * VS >= 6 * VM_THREADS, "one record per thread; the bbox reduction borrows the tile");

struct VolMultiArgs {
    vpho_obj_solids s;
    vpho_obj_solid_columns c;
    const int* faces;            // (F, 3)
    int F;
    const float* verts;          // (n, S, V, 3)
    const double* rt;            // (n, S, 3, 4)
    const int* obj_id;           // (n,)
    int n, S, V;
    double cell_volume;          // (h * h) * h
    double* per_hyp;             // (n, S, 2) n_cells | IV
    double* table;               // (n, 6)
    unsigned char* flags;        // (n, S, max_pts) or NULL; zeroed by the host
};

__global__ __launch_bounds__(VM_THREADS) void column_walk_kernel(const VolMultiArgs a) {
    __shared__ double tile[VM_TILE * VS];
    __shared__ double s_box[6];
    __shared__ int2 s_item[2 * VM_THREADS];            // (first centre, number of centres <= VM_PIECE)
    __shared__ int s_n, s_cells;
    const long long pair = blockIdx.x;                 // image * S + hypothesis
    const int img = (int)(pair / a.S), tid = threadIdx.x;
    double* out = a.per_hyp + pair * 2;
    const int o = a.obj_id[img];
    if (!(o >= 0 && o < a.s.n_obj)) {                  // the whole workgroup: NaN, as volume_finish_kernel
        if (tid < 2) out[tid] = NAN;
        return;
    }
    const double* R = a.rt + pair * 12;
    const float* verts = a.verts + pair * a.V * 3;
    // ---- bbox of the face corners (hand_mesh_setup_kernel pass 1)
    double* s_lo = tile;
    double* s_hi = tile + 3 * VM_THREADS;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    int bad = 0;
    for (int f = tid; f < a.F; f += VM_THREADS) {
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
    for (int k = 0; k < 3; ++k) { s_lo[k * VM_THREADS + tid] = lo[k]; s_hi[k * VM_THREADS + tid] = hi[k]; }
    bad = __syncthreads_or(bad);
    for (int h = VM_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                s_lo[k * VM_THREADS + tid] = fmin(s_lo[k * VM_THREADS + tid], s_lo[k * VM_THREADS + tid + h]);
                s_hi[k * VM_THREADS + tid] = fmax(s_hi[k * VM_THREADS + tid], s_hi[k * VM_THREADS + tid + h]);
            }
        }
        __syncthreads();
    }
    if (tid < 3) {
        // MeshIntersector.__init__: scale = (resolution - 1) / (bbox_max - bbox_min), translate = 0.5 - scale * bbox_min
        const double sc = (double)(VPHO_PEN_RESOLUTION - 1) / (s_hi[tid * VM_THREADS] - s_lo[tid * VM_THREADS]);
        s_box[tid] = sc;
        s_box[3 + tid] = 0.5 - sc * s_lo[tid * VM_THREADS];
    }
    if (tid == 0) { s_n = 0; s_cells = 0; }
    __syncthreads();
    if (bad) {                                         // no record is built: a bad face index is never dereferenced
        if (tid < 2) out[tid] = NAN;
        return;
    }
    const int pb = a.s.pt_offset[o], pe = a.s.pt_offset[o + 1];
    const int cb = a.c.col_offset[o], ncol = a.c.col_offset[o + 1] - cb;

    // the workgroup walks the last min(s_n, 256) pieces of the list through all faces; s_n is stable on entry (behind a barrier)
    auto walk = [&]() {
        const int total = s_n, cnt = min(total, VM_THREADS), base = total - cnt;
        const bool mine = tid < cnt;
        int start = 0, len = 0;
        float x = 0.f, y = 0.f;
        double qx = -1.0, qy = -1.0, cx = -1.0, cy = -1.0;
        if (mine) {
            const int2 it = s_item[base + tid];
            start = it.x; len = it.y;
            const float* c = a.s.pts + (long long)start * 3;
            x = c[0]; y = c[1];
            double qz;
            pen_hash_frame(s_box, s_box + 3, (double)x, (double)y, (double)c[2], qx, qy, qz);
            pen_cell(qx, qy, 0.0, cx, cy);             // the column's cell: that of every centre of it that has one
        }
        unsigned long long m0 = 0, m1 = 0;
        for (int t0 = 0; t0 < a.F; t0 += VM_TILE) {
            const int tc = min(VM_TILE, a.F - t0);
            __syncthreads();                           // the tile's last readers (first tile: the bbox arrays, the list)
            if (tid < tc) {
                // the 19 parity fields of face t0 + tid (hand_mesh_setup_kernel pass 2)
                double t[3][3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    double px, py, pz;
                    pen_model_frame(R, verts + (long long)a.faces[3 * (t0 + tid) + c] * 3, px, py, pz);
                    pen_hash_frame(s_box, s_box + 3, px, py, pz, t[c][0], t[c][1], t[c][2]);
                }
                pen_face_record(t, tile + tid * VS);
            }
            __syncthreads();
            if (!mine) continue;
            for (int k = 0; k < tc; ++k) {
                const double* r = tile + k * VS;
                double depth;
                if (!pen_parity_xy(r, qx, qy, cx, cy, depth)) continue;
                for (int j = 0; j < len; ++j) {
                    double ux, uy, qz, ccx, ccy;
                    pen_hash_frame(s_box, s_box + 3, (double)x, (double)y, (double)a.s.pts[((long long)start + j) * 3 + 2], ux, uy, qz);
                    if (!pen_cell(ux, uy, qz, ccx, ccy)) continue;            // the [0, 512]^3 cull of this centre
                    unsigned p0 = 0, p1 = 0;
                    pen_parity_z(r, depth, qz, p0, p1);
                    m0 ^= (unsigned long long)p0 << j;
                    m1 ^= (unsigned long long)p1 << j;
                }
            }
        }
        unsigned long long ins = m0 & m1;
        const int c = __popcll(ins);
        if (c) atomicAdd(&s_cells, c);
        if (a.flags) {
            unsigned char* fl = a.flags + pair * a.s.max_pts + (start - pb);
            while (ins) {
                fl[__ffsll((long long)ins) - 1] = 1;
                ins &= ins - 1;
            }
        }
        __syncthreads();
        if (tid == 0) s_n = base;
        __syncthreads();
    };

    for (int w = 0; w < ncol; w += VM_THREADS) {
        const int col = w + tid;
        int start = 0, end = 0;
        bool live = false;
        if (col < ncol) {
            start = max(a.c.col_start[cb + col], pb);
            end = min(a.c.col_start[cb + col + 1], pe);
            if (start < end) {
                const float* c = a.s.pts + (long long)start * 3;
                double qx, qy, qz, cx, cy;
                pen_hash_frame(s_box, s_box + 3, (double)c[0], (double)c[1], (double)c[2], qx, qy, qz);
                live = pen_cell(qx, qy, 0.0, cx, cy);  // no cell in x, y: none of the column's centres has one
            }
        }
        for (int p0 = start; ; p0 += VM_PIECE) {
            const bool has = live && p0 < end;
            if (!__syncthreads_or(has ? 1 : 0)) break;
            if (has) s_item[atomicAdd(&s_n, 1)] = make_int2(p0, min(VM_PIECE, end - p0));
            __syncthreads();
            if (s_n >= VM_THREADS) walk();
        }
    }
    if (s_n > 0) walk();
    if (tid == 0) {
        const double cells = (double)s_cells;
        out[0] = cells;
        out[1] = a.cell_volume * cells;
    }
}

// one thread per image: one = hypothesis 0; best = the minima; mean_cells = (integer sum) / S, mean_IV = cell_volume * mean_cells
__global__ __launch_bounds__(256) void volume_table_kernel(const VolMultiArgs a) {
    const int img = blockIdx.x * 256 + threadIdx.x;
    if (img >= a.n) return;
    const double* src = a.per_hyp + (long long)img * a.S * 2;
    bool nan = false;
    long long sum = 0;
    double lo_cells = INFINITY, lo_iv = INFINITY;
    for (int s = 0; s < a.S; ++s) {
        const double cells = src[2 * s], iv = src[2 * s + 1];
        if (cells != cells || iv != iv) { nan = true; continue; }
        sum += (long long)cells;
        lo_cells = fmin(lo_cells, cells);
        lo_iv = fmin(lo_iv, iv);
    }
    const double mean_cells = (double)sum / (double)a.S;
    double* out = a.table + (long long)img * 6;
    out[0] = src[1];
    out[1] = src[0];
    out[2] = nan ? NAN : lo_iv;
    out[3] = nan ? NAN : lo_cells;
    out[4] = nan ? NAN : a.cell_volume * mean_cells;
    out[5] = nan ? NAN : mean_cells;
}

}  // namespace

extern "C" long long vpho_hand_obj_intersection_multi_workspace_bytes(int n, int S, int F) {
    if (n < 0 || S < 1 || F <= 0 || (long long)n * S > 0x7fffffffLL) return -1;
    return 0;                                          // the records live in LDS and the parities in registers
}

extern "C" int vpho_hand_obj_intersection_multi_f64(const vpho_obj_mesh_tables* t, const vpho_obj_solids* solids, const vpho_obj_solid_columns* cols,
                                                    const int* faces, int F, const float* verts, int n, int S, int V, const double* obj_rt,
                                                    const int* obj_id, double pitch, double* per_hyp, double* table, unsigned char* flags,
                                                    void* workspace, long long workspace_bytes_given, void* stream) {
    (void)workspace; (void)workspace_bytes_given;
    VPHO_REQUIRE(t && t->n_obj > 0, "vpho_hand_obj_intersection_multi_f64: bad mesh tables");
    VPHO_REQUIRE(solids && solids->pts && solids->pt_offset && solids->n_obj == t->n_obj && solids->max_pts >= 0,
                 "vpho_hand_obj_intersection_multi_f64: bad solid tables (they must cover the %d objects of the mesh tables)", t->n_obj);
    VPHO_REQUIRE(cols && cols->col_start && cols->col_offset && cols->n_obj == t->n_obj && cols->max_cols >= 0,
                 "vpho_hand_obj_intersection_multi_f64: bad column tables (they must cover the %d objects of the mesh tables)", t->n_obj);
    VPHO_REQUIRE(S >= 1, "vpho_hand_obj_intersection_multi_f64: no hypotheses (S=%d)", S);
    VPHO_REQUIRE(F > 0, "vpho_hand_obj_intersection_multi_f64: a hand mesh without faces (F=%d)", F);
    VPHO_REQUIRE(pitch > 0.0, "vpho_hand_obj_intersection_multi_f64: the voxel pitch must be positive (%g)", pitch);
    VPHO_REQUIRE(n >= 0 && V > 0, "vpho_hand_obj_intersection_multi_f64: bad shape (n=%d, V=%d)", n, V);
    VPHO_REQUIRE((long long)n * S <= 0x7fffffffLL, "vpho_hand_obj_intersection_multi_f64: n * S = %lld pairs, at most 2147483647 (one workgroup each on grid.x)",
                 (long long)n * S);
    if (n == 0) return 0;
    VPHO_REQUIRE(faces && verts && obj_rt && obj_id && per_hyp && table, "vpho_hand_obj_intersection_multi_f64: bad argument");
    hipStream_t s = (hipStream_t)stream;
    VolMultiArgs a;
    a.s = *solids; a.c = *cols; a.faces = faces; a.F = F; a.verts = verts; a.rt = obj_rt; a.obj_id = obj_id; a.n = n; a.S = S; a.V = V;
    a.cell_volume = (pitch * pitch) * pitch;
    a.per_hyp = per_hyp; a.table = table; a.flags = flags;
    if (flags && solids->max_pts > 0) VPHO_HIP(hipMemsetAsync(flags, 0, (size_t)n * S * solids->max_pts, s));
    hipLaunchKernelGGL(column_walk_kernel, dim3((unsigned)((long long)n * S)), dim3(VM_THREADS), 0, s, a);
    int rc = vpho::check_launch("column_walk_kernel");
    if (!rc) {
        hipLaunchKernelGGL(volume_table_kernel, dim3((n + 255) / 256), dim3(256), 0, s, a);
        rc = vpho::check_launch("volume_table_kernel");
    }
    return rc;
}
