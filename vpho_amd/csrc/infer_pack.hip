// Prediction records of --mode infer (Trainer.infer, lib/engine/train_diff_hand_obj.py:359-444): one launch per batch turns the predict
// outputs into fixed-layout per-image records (include/vpho_hip.h, vpho_infer_pack_f32), one hipMemcpyAsync ships them to the host.
//   block A  fp32  reg_joint | reg_vert | agg_joint | agg_vert in the camera frame: __postprocess_hand_vert (:598-602), x negated for
//                  left hands, then + root_joint -- one sign flip (exact) and one fp32 add per element, so the bits are defined
//   block B  fp16  agg_vert of block A, `.astype(np.float16)` (:383): round to nearest even, overflow to inf, subnormals kept
//   block C  fp64  pd_obj_rt = obj_9D_to_mat + root (:593-596) by vpho::obj_9d_to_rt, the function behind vpho_obj_9d_to_rt_f64
// HBM-bound by its bytes (19 KB read, 24 KB written per image) but only ~3 MB at the README batch of 64: the launch is latency-bound.
// Flat walk over PAIRS of block-A elements: a lane reads two dwords (adjacent lanes adjacent addresses: whole-wave coalesced 256 B
// rows), writes one dwordx2 of block A and, in the agg_vert segment, one dword holding two halves of block B.  No atomics, no LDS.
#include "common.h"
#include "rot.h"
#include "../../include/vpho_hip.h"

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

__host__ __device__ inline long long rec_a_floats(int nj, int nv) { return 6LL * (nj + nv); }
__host__ __device__ inline long long rec_b_offset(int nj, int nv) { return rec_a_floats(nj, nv) * 4; }
__host__ __device__ inline long long rec_c_offset(int nj, int nv) { return (rec_b_offset(nj, nv) + 6LL * nv + 7) / 8 * 8; }
__host__ __device__ inline long long rec_bytes(int nj, int nv) { return rec_c_offset(nj, nv) + 96; }

struct PackArgs {
    const float *reg_j, *reg_v, *agg_j, *agg_v;
    const double* obj9;
    const float* root;
    const unsigned char* is_right;
    int n, nj, nv;
    char* rec;
};

// element e (0 <= e < 6 (nj + nv)) of image b's block A; every segment starts at a multiple of 3, so the component is e % 3
__device__ __forceinline__ float block_a_value(const PackArgs& a, int b, unsigned e, float sgn, const float* root3) {
    const unsigned J = 3u * a.nj, V = 3u * a.nv;
    const float* src;
    unsigned k, len;
    if (e < J) { src = a.reg_j; k = e; len = J; }
    else if (e < J + V) { src = a.reg_v; k = e - J; len = V; }
    else if (e < 2 * J + V) { src = a.agg_j; k = e - J - V; len = J; }
    else { src = a.agg_v; k = e - 2 * J - V; len = V; }
    const unsigned c = e % 3u;
    const float v = src[(long long)b * len + k];
    return (c == 0 ? sgn * v : v) + root3[c];
}

__global__ __launch_bounds__(256) void infer_pack_kernel(PackArgs a) {
    const unsigned per = (unsigned)(rec_a_floats(a.nj, a.nv) / 2);        // pairs per image
    const unsigned agg_v0 = 3u * (2u * a.nj + a.nv);                        // first element of the agg_vert segment (even: nv is even)
    const long long rb = rec_bytes(a.nj, a.nv), boff = rec_b_offset(a.nj, a.nv);
    const long long total = (long long)a.n * per;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
    for (long long i = gid; i < total; i += stride) {
        const int b = (int)(i / per);
        const unsigned e = 2u * (unsigned)(i - (long long)b * per);
        const float sgn = a.is_right[b] ? 1.f : -1.f;
        const float* root3 = a.root + (long long)b * 3;
        f32x2 v;
        v.x = block_a_value(a, b, e, sgn, root3);
        v.y = block_a_value(a, b, e + 1, sgn, root3);
        char* r = a.rec + (long long)b * rb;
        *reinterpret_cast<f32x2*>(r + 4LL * e) = v;
        if (e >= agg_v0) *reinterpret_cast<f16x2*>(r + boff + 2LL * (e - agg_v0)) = __builtin_convertvector(v, f16x2);
    }
    // block C and the padding behind block B: one thread per image
    for (long long b = gid; b < a.n; b += stride) {
        char* r = a.rec + b * rb;
        const long long bend = boff + 6LL * a.nv, coff = rec_c_offset(a.nj, a.nv);
        if (coff - bend >= 4) *reinterpret_cast<unsigned*>(r + bend) = 0u;           // bend is a multiple of 4: the gap is 0 or 4 bytes
        vpho::obj_9d_to_rt(a.obj9 + b * 9, a.root + b * 3, reinterpret_cast<double*>(r + coff));
    }
}

}  // namespace

extern "C" long long vpho_infer_record_bytes(int n_joint, int n_vert) {
    if (n_joint <= 0 || n_vert <= 0 || (n_vert & 1) || n_joint > (1 << 20) || n_vert > (1 << 20)) return -1;
    return rec_bytes(n_joint, n_vert);
}

extern "C" int vpho_infer_pack_f32(const float* reg_hand_joint, const float* reg_hand_vert, const float* agg_hand_joint, const float* agg_hand_vert,
                                   const double* agg_obj_6d, const float* root_joint, const unsigned char* is_right, int n_img, int n_joint,
                                   int n_vert, void* records, void* records_host, void* stream) {
    VPHO_REQUIRE(reg_hand_joint && reg_hand_vert && agg_hand_joint && agg_hand_vert && agg_obj_6d && root_joint && is_right && records,
                 "vpho_infer_pack_f32: null pointer");
    VPHO_REQUIRE(n_img > 0 && n_img <= (1 << 20), "vpho_infer_pack_f32: n_img = %d out of range", n_img);
    VPHO_REQUIRE(vpho_infer_record_bytes(n_joint, n_vert) > 0, "vpho_infer_pack_f32: n_joint = %d, n_vert = %d (both positive, n_vert even)", n_joint, n_vert);
    VPHO_REQUIRE(((uintptr_t)records & 7) == 0 && ((uintptr_t)records_host & 7) == 0, "vpho_infer_pack_f32: records must be 8-byte aligned");
    PackArgs a{reg_hand_joint, reg_hand_vert, agg_hand_joint, agg_hand_vert, agg_obj_6d, root_joint, is_right, n_img, n_joint, n_vert, (char*)records};
    const long long pairs = (long long)n_img * (rec_a_floats(n_joint, n_vert) / 2);
    const long long blocks = (pairs + 255) / 256;
    hipLaunchKernelGGL(infer_pack_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, (hipStream_t)stream, a);
    if (int rc = vpho::check_launch("infer_pack_kernel")) return rc;
    if (records_host)
        VPHO_HIP(hipMemcpyAsync(records_host, records, (size_t)(n_img * rec_bytes(n_joint, n_vert)), hipMemcpyDeviceToHost, (hipStream_t)stream));
    return 0;
}
