// The reference's ablation aggregators (lib/model/aggregation.py HandAggregator :82-113,286-467, ObjectAggregator :646-659,1001-1112;
// INTEGRATION.md 1): what the modes other than `heatmap_cascade` need beyond the cascade's own kernels (aggregate.hip) -- the heat-map
// peak of the 2D_pt modes, the distance of the projected joints / key-points to it, the quaternion mean of WHOLE poses over an index
// list, the per-joint mean of 2D_pt_joint.  Small, latency-bound launches: one wavefront per heat map, one lane per (image, candidate)
// or per (image, joint).  Every sum runs in a fixed order (no float atomics): two calls on the same input give the same bits.
#include "common.h"
#include "rot.h"
#include "../../include/vpho_hip.h"

namespace {

inline int nblocks(long long n, int bs = 256) { return (int)((n + bs - 1) / bs); }

// pinhole projection (aggregation.py:24-32) then normalisation to the bbox (:308-311, :1020-1023): the operations of aggregate.hip's
// project_norm / project_norm_d, which the cascade's scores use
__device__ inline void project_norm(const float* p3, const float* K, const float* bbox, float& gx, float& gy) {
    const float u = p3[0] * K[0] + p3[1] * K[1] + p3[2] * K[2];
    const float v = p3[0] * K[3] + p3[1] * K[4] + p3[2] * K[5];
    const float w = p3[0] * K[6] + p3[1] * K[7] + p3[2] * K[8];
    const float px = u / w - bbox[0], py = v / w - bbox[1];
    gx = 2.f * px / (bbox[2] - bbox[0]) - 1.f;
    gy = 2.f * py / (bbox[3] - bbox[1]) - 1.f;
}
__device__ inline void project_norm_d(const double* p3, const float* K, const float* bbox, double& gx, double& gy) {
    const double u = p3[0] * (double)K[0] + p3[1] * (double)K[1] + p3[2] * (double)K[2];
    const double v = p3[0] * (double)K[3] + p3[1] * (double)K[4] + p3[2] * (double)K[5];
    const double w = p3[0] * (double)K[6] + p3[1] * (double)K[7] + p3[2] * (double)K[8];
    const double px = u / w - (double)bbox[0], py = v / w - (double)bbox[1];
    gx = 2.0 * px / ((double)bbox[2] - (double)bbox[0]) - 1.0;
    gy = 2.0 * py / ((double)bbox[3] - (double)bbox[1]) - 1.0;
}

// ---------------------------------------------------------------------------------------- heat-map peak (aggregation.py:313-323)
// torch.argmax order: the larger value wins, a NaN beats every number, equal values (or two NaNs): the smaller index
__device__ inline bool peak_before(float v, int i, float bv, int bi) {
    const bool vn = v != v, bn = bv != bv;
    if (vn != bn) return vn;
    if (!vn && v != bv) return v > bv;
    return i < bi;
}
// One wavefront per (image, channel) map of side x side values.  The reference reads the peak's coordinates out of torch.meshgrid(X, Y)
// (`ij` order) flattened against the row-major map: the value it uses as x is X[ind / side], as y Y[ind % side] -- a transposition,
// kept; X[i] = i / (side - 1) * 2 - 1 in fp32.
__global__ __launch_bounds__(64) void heatmap_peak_kernel(const float* __restrict__ heatmap, int side, float* __restrict__ peak, int* __restrict__ ind) {
    const long long m = blockIdx.x;
    const float* plane = heatmap + m * side * side;
    const int lane = threadIdx.x, n = side * side;
    float best = -INFINITY; int bi = 0x7fffffff;
    for (int i = lane; i < n; i += 64) {
        const float v = plane[i];
        if (bi == 0x7fffffff || peak_before(v, i, best, bi)) { best = v; bi = i; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o); const int oi = __shfl_xor(bi, o);
        if (oi != 0x7fffffff && (bi == 0x7fffffff || peak_before(ob, oi, best, bi))) { best = ob; bi = oi; }
    }
    if (lane == 0) {
        const float d = (float)(side - 1);
        peak[m * 2 + 0] = (float)(bi / side) / d * 2.f - 1.f;
        peak[m * 2 + 1] = (float)(bi % side) / d * 2.f - 1.f;
        if (ind) ind[m] = bi;
    }
}

// ---------------------------------------------------------------------------------------- 2-D point scores (aggregation.py:303-327)
// hand: score[b][c][j] = -|| norm_to_bbox(project(joint[b][c][j] + root[b])) - peak[b][j] ||, fp32 in the reference's operation order;
// PER_JOINT: the (bs, C, 21) matrix (vpho_topk_f32 with F = 21), else its sum over the joints in ascending order (bs, C)
template <bool PER_JOINT>
__global__ void hand_pt2d_kernel(const float* __restrict__ joints, const float* __restrict__ root, const float* __restrict__ Kmat,
                                 const float* __restrict__ bbox, const float* __restrict__ peak, int bs, int C, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)bs * C) return;
    const int b = (int)(i / C);
    float acc = 0.f;
    for (int j = 0; j < 21; ++j) {
        const float* p = joints + (i * 21 + j) * 3;
        const float p3[3] = {p[0] + root[b * 3 + 0], p[1] + root[b * 3 + 1], p[2] + root[b * 3 + 2]};
        float gx, gy;
        project_norm(p3, Kmat + b * 9, bbox + b * 4, gx, gy);
        const float dx = gx - peak[(b * 21 + j) * 2 + 0], dy = gy - peak[(b * 21 + j) * 2 + 1];
        const float s = -sqrtf(dx * dx + dy * dy);
        if (PER_JOINT) out[i * 21 + j] = s; else acc += s;
    }
    if (!PER_JOINT) out[i] = acc;
}

// object: score[b][c] = -sum_j || norm_to_bbox(project(flip(R(pose) kpt_j + t + root))) - peak[b][j] ||      (aggregation.py:1015-1039)
// the poses are fp64 (quirk Q5): the whole chain in double like aggregate.hip's obj_heat_kernel<true>, one rounding at the end
__global__ void obj_pt2d_kernel(const double* __restrict__ pose, const float* __restrict__ root, const float* __restrict__ kpt_tab,
                                const int* __restrict__ obj_id, const unsigned char* __restrict__ is_right, const float* __restrict__ Kmat,
                                const float* __restrict__ bbox, const float* __restrict__ peak, int bs, int n, int J, int n_obj, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)bs * n) return;
    const int b = (int)(i / n);
    const int oid = obj_id[b];
    if (oid < 0 || oid >= n_obj) { out[i] = NAN; return; }            // an unknown class: no table row to read
    const double* pp = pose + i * 9;
    const float* kp = kpt_tab + (long long)oid * J * 3;
    double R[9], t[3];
    vpho::rot6d_to_matrix<double>(pp, R);
    for (int k = 0; k < 3; ++k) t[k] = pp[6 + k] + (double)root[b * 3 + k];
    const double sgn = is_right[b] ? 1.0 : -1.0;
    double acc = 0.0;
    for (int j = 0; j < J; ++j) {
        double p3[3];
        for (int r = 0; r < 3; ++r) p3[r] = ((double)kp[j * 3 + 0] * R[r * 3 + 0] + (double)kp[j * 3 + 1] * R[r * 3 + 1] + (double)kp[j * 3 + 2] * R[r * 3 + 2]) + t[r];
        p3[0] = p3[0] * sgn;
        double gx, gy;
        project_norm_d(p3, Kmat + b * 9, bbox + b * 4, gx, gy);
        const double dx = gx - (double)peak[((long long)b * J + j) * 2 + 0], dy = gy - (double)peak[((long long)b * J + j) * 2 + 1];
        acc += -sqrt(dx * dx + dy * dy);
    }
    out[i] = (float)acc;
}

// ---------------------------------------------------------------------------------------- whole-pose fuse (aggregation.py:221-233,331-336,401-405)
// One lane per (image, MANO rotation): the quaternion mean (transform_fn.average_quaternion) of that rotation over the n listed
// candidates, in list order -- the moment matrix sum_r w_r q_r q_r^T / sum_r w_r with the operations of aggregate.hip's hand_fuse_kernel
// and the shared sym4_top_eigenvector.  idx NULL: candidates 0 .. n-1; w NULL: every weight 1 (the reference's W = ones).
struct PoseFuseArgs {
    const float* pose; int ld, C;                 // rows of ld floats (first 48 = axis-angle), C candidates per image
    const int* idx; const float* w;               // (bs, n) each, optional
    int bs, n;
    float* out;                                   // (bs, 48)
};
__global__ __launch_bounds__(64) void hand_pose_fuse_kernel(const PoseFuseArgs a) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.bs * 16) return;
    const int b = t / 16, joint = t % 16;
    float A[4][4] = {{0}};
    float wsum = 0.f;
    bool bad = false;
    for (int r = 0; r < a.n; ++r) {
        const int c = a.idx ? a.idx[(long long)b * a.n + r] : r;
        if (c < 0 || c >= a.C) { bad = true; continue; }             // never read outside the candidates
        const float wr = a.w ? a.w[(long long)b * a.n + r] : 1.f;
        const float* aa = a.pose + ((long long)b * a.C + c) * a.ld + joint * 3;
        float q[4];
        vpho::axis_angle_to_quaternion(aa, q);
        const float sg = q[0] > 0.f ? 1.f : -1.f;
        for (int i = 0; i < 4; ++i) q[i] *= sg;
        for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) A[i][j] += (q[i] * q[j]) * wr;
        wsum += wr;
    }
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) A[i][j] /= wsum;
    float qa[4], aa[3];
    vpho::sym4_top_eigenvector(A, qa);
    const float sg = qa[0] > 0.f ? 1.f : -1.f;
    for (int i = 0; i < 4; ++i) qa[i] *= sg;
    vpho::quaternion_to_axis_angle(qa, aa);
    for (int e = 0; e < 3; ++e) a.out[(long long)b * 48 + joint * 3 + e] = bad ? NAN : aa[e];
}

// 2D_pt_joint (aggregation.py:357-362): fused joint j = mean over the k candidates selected FOR THAT JOINT; idx [b][21][k] as vpho_topk_f32
// with F = 21 writes it; the sum in list order, then / k (torch.mean)
__global__ void joint_gather_mean_kernel(const float* __restrict__ joints, const int* __restrict__ idx, int bs, int C, int k, float* __restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= bs * 63) return;
    const int b = t / 63, j = (t % 63) / 3, e = t % 3;
    float acc = 0.f;
    bool bad = false;
    for (int r = 0; r < k; ++r) {
        const int c = idx[((long long)b * 21 + j) * k + r];
        if (c < 0 || c >= C) { bad = true; continue; }
        acc += joints[(((long long)b * C + c) * 21 + j) * 3 + e];
    }
    out[t] = bad ? NAN : acc / (float)k;
}

}  // namespace

extern "C" int vpho_heatmap_peak_f32(const float* heatmap, long long n_maps, int H, int W, float* peak, int* ind, void* stream) {
    VPHO_REQUIRE(heatmap && peak && n_maps > 0 && n_maps <= 0x7fffffffLL && H > 1 && H <= 32768, "vpho_heatmap_peak_f32: bad argument");
    VPHO_REQUIRE(H == W, "vpho_heatmap_peak_f32: the 2D_pt aggregation modes need square heat maps (got %d x %d): the reference reads the "
                         "peak through a transposed grid that is only defined for H = W", H, W);
    hipLaunchKernelGGL(heatmap_peak_kernel, dim3((unsigned)n_maps), dim3(64), 0, (hipStream_t)stream, heatmap, H, peak, ind);
    return vpho::check_launch("heatmap_peak_kernel");
}

extern "C" int vpho_hand_pt2d_score_f32(const float* joints, const float* root, const float* Kmat, const float* bbox, const float* peak,
                                        int bs, int C, int per_joint, float* score, void* stream) {
    VPHO_REQUIRE(joints && root && Kmat && bbox && peak && score && bs > 0 && C > 0, "vpho_hand_pt2d_score_f32: bad argument");
    const dim3 grid(nblocks((long long)bs * C)), block(256);
    if (per_joint) hipLaunchKernelGGL(hand_pt2d_kernel<true>, grid, block, 0, (hipStream_t)stream, joints, root, Kmat, bbox, peak, bs, C, score);
    else hipLaunchKernelGGL(hand_pt2d_kernel<false>, grid, block, 0, (hipStream_t)stream, joints, root, Kmat, bbox, peak, bs, C, score);
    return vpho::check_launch("hand_pt2d_kernel");
}

extern "C" int vpho_obj_pt2d_score(const double* pose, int n, const float* root, const vpho_obj_tables* t, const int* obj_id,
                                   const unsigned char* is_right, const float* Kmat, const float* bbox, const float* peak, int bs,
                                   float* score, void* stream) {
    VPHO_REQUIRE(pose && root && t && t->kpt && obj_id && is_right && Kmat && bbox && peak && score && bs > 0 && n > 0 && t->n_kpt > 0 && t->n_obj > 0,
                 "vpho_obj_pt2d_score: bad argument");
    hipLaunchKernelGGL(obj_pt2d_kernel, dim3(nblocks((long long)bs * n)), dim3(256), 0, (hipStream_t)stream, pose, root, t->kpt, obj_id, is_right,
                       Kmat, bbox, peak, bs, n, t->n_kpt, t->n_obj, score);
    return vpho::check_launch("obj_pt2d_kernel");
}

extern "C" int vpho_hand_pose_fuse_f32(const float* pose, int ld_pose, int C, const int* idx, const float* w, int bs, int n, float* fused,
                                       void* stream) {
    VPHO_REQUIRE(pose && fused && bs > 0 && C > 0 && ld_pose >= 48, "vpho_hand_pose_fuse_f32: bad argument");
    VPHO_REQUIRE(n > 0 && (idx ? n <= 2 * C : n <= C), "vpho_hand_pose_fuse_f32: %d candidates to fuse out of %d", n, C);
    PoseFuseArgs a;
    a.pose = pose; a.ld = ld_pose; a.C = C; a.idx = idx; a.w = w; a.bs = bs; a.n = n; a.out = fused;
    hipLaunchKernelGGL(hand_pose_fuse_kernel, dim3(nblocks((long long)bs * 16, 64)), dim3(64), 0, (hipStream_t)stream, a);
    return vpho::check_launch("hand_pose_fuse_kernel");
}

extern "C" int vpho_hand_joint_gather_mean_f32(const float* joints, const int* idx, int bs, int C, int k, float* fused, void* stream) {
    VPHO_REQUIRE(joints && idx && fused && bs > 0 && C > 0 && k > 0 && k <= C, "vpho_hand_joint_gather_mean_f32: bad argument");
    hipLaunchKernelGGL(joint_gather_mean_kernel, dim3(nblocks((long long)bs * 63)), dim3(256), 0, (hipStream_t)stream, joints, idx, bs, C, k, fused);
    return vpho::check_launch("joint_gather_mean_kernel");
}
