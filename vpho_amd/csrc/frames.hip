// The data front end on the device: what the reference's Dataset.__getitem__ does per image on CPU workers, as two launches per batch.
//   frame_patch_kernel      lib/dataset/dexycb6.py:345 (cv2.warpAffine, INTER_CUBIC, constant border 0), :389-391 (RGBShift, brightness and
//                           saturation of ColorJitter), :398-399 (left hands mirrored), :442-444 (normalize_rgb, timm RandomErasing 'pixel')
//   heatmap_targets_kernel  lib/utils/misc_fn.py:285-385 (HeatmapGenerator.get_heatmap, AdaptiveHeatmapGenerator.__call__)
// Both are one thread per output pixel, no LDS, no atomics; every index into the frame, the Gaussian table and the output is checked.
#include "common.h"
#include "frames_common.h"
#include "../../include/vpho_hip.h"
#include <cstdint>

namespace {

// ---------------------------------------------------------------------------------------------------------------- warp + colour
struct PatchArgs {
    const unsigned char* frames; const double* minv; const float* colour; const unsigned char* flip; const int* erase; const unsigned int* key;
    float* out; int H, W, P;
};

__global__ __launch_bounds__(256) void frame_patch_kernel(const PatchArgs a) {
    const int P = a.P, s = blockIdx.y;
    const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;            // consecutive lanes = consecutive x of one output row
    if (pix >= (long long)P * P) return;
    const int y = (int)(pix / P), x = (int)(pix % P);
    const bool flip = a.flip && a.flip[s];
    const int xs = flip ? P - 1 - x : x;                                         // the patch column that lands here
    float v[3];
    bicubic_crop(a.frames + (long long)s * a.H * a.W * 3, a.H, a.W, a.minv + 6 * (long long)s, xs, y, v);
    if (a.colour) {                                                              // every stage ends on an integer grey level
        const float* c = a.colour + 5 * (long long)s;
        const float b = c[3], sat = c[4];
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = level(v[k] + c[k]);
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = level(v[k] * b);
        const float gray = level((0.299f * v[0] + 0.587f * v[1]) + 0.114f * v[2]);
        const float g1 = (1.f - sat) * gray;
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = level(sat * v[k] + g1);
    }
    float o[3];
    normalise_erase(v, a.erase, a.key, s, x, y, pix, o);
    float* q = a.out + (long long)s * 3 * P * P + pix;
    q[0] = o[0];
    q[(long long)P * P] = o[1];
    q[2ll * P * P] = o[2];
}

// ---------------------------------------------------------------------------------------------------------------- heat-map targets
// one joint's stamp of the reference's generators, evaluated at one cell (u, v) of a map of rw x rh cells: the Gaussian table g (G x G)
// placed with its corner at ul = rint(x - 3 sigma - 1) (x = the joint's coordinate truncated toward zero), clipped to the map
struct Stamp { int ok, ulx, uly, brx, bry; };
__device__ __forceinline__ Stamp make_stamp(double px, double py, int rw, int rh, double sigma) {
    Stamp st{0, 0, 0, 0, 0};
    if (!(fabs(px) < 1e9 && fabs(py) < 1e9)) return st;                          // not finite, or beyond any map
    const int x = (int)px, y = (int)py;                                          // int(): toward zero
    if (x < 0 || y < 0 || x >= rw || y >= rh) return st;
    st.ok = 1;
    st.ulx = (int)rint(((double)x - 3.0 * sigma) - 1.0);                         // np.round: half to even
    st.uly = (int)rint(((double)y - 3.0 * sigma) - 1.0);
    st.brx = min((int)rint(((double)x + 3.0 * sigma) + 2.0), rw);
    st.bry = min((int)rint(((double)y + 3.0 * sigma) + 2.0), rh);
    return st;
}
__device__ __forceinline__ float stamp_at(const Stamp& st, int u, int v, const float* __restrict__ g, int G) {
    if (!st.ok || u < max(st.ulx, 0) || u >= st.brx || v < max(st.uly, 0) || v >= st.bry) return 0.f;
    const int gx = u - st.ulx, gy = v - st.uly;
    return (gx >= 0 && gx < G && gy >= 0 && gy < G) ? g[gy * G + gx] : 0.f;
}
// cv2.resize(INTER_LINEAR): source of destination cell d = (d + 0.5) * res / S - 0.5, the two taps clamped to the edge
__device__ __forceinline__ void linear_taps(int d, int res, int S, int& i0, int& i1, float& t) {
    const double f = ((double)d + 0.5) * (double)res / (double)S - 0.5;
    const double fl = floor(f);
    t = (float)(f - fl);
    const int i = (int)fl;
    i0 = min(max(i, 0), res - 1);
    i1 = min(max(i + 1, 0), res - 1);
}

__global__ __launch_bounds__(256) void heatmap_targets_kernel(const double* __restrict__ pts, const double* __restrict__ box, const int* __restrict__ res,
                                                              const unsigned char* __restrict__ left, const float* __restrict__ g, int G, double sigma,
                                                              double gmin, int J, int S, int adaptive, float* __restrict__ out, long long total) {
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= total) return;
    const int u = (int)(id % S), v = (int)((id / S) % S);
    const long long sj = id / ((long long)S * S);                                // sample * J + joint
    const int s = (int)(sj / J);
    const double* b = box + 4 * (long long)s;
    const double ptx = pts[2 * sj], pty = pts[2 * sj + 1];
    float val;
    if (!adaptive) {
        double px = (ptx - b[0]) / b[2] * (double)(S - 1);
        const double py = (pty - b[1]) / b[2] * (double)(S - 1);
        if (left && left[s]) px = px + 1.0;
        val = stamp_at(make_stamp(px, py, S, S, sigma), u, v, g, G);
    } else {
        const int rw = res[2 * s], rh = res[2 * s + 1];
        const Stamp st = make_stamp((ptx - b[0]) * (double)rw / b[2], (pty - b[1]) * (double)rh / b[3], rw, rh, sigma);
        int x0, x1, y0, y1;
        float tx, ty;
        linear_taps(u, rw, S, x0, x1, tx);
        linear_taps(v, rh, S, y0, y1, ty);
        const float top = (1.f - tx) * stamp_at(st, x0, y0, g, G) + tx * stamp_at(st, x1, y0, g, G);
        const float bot = (1.f - tx) * stamp_at(st, x0, y1, g, G) + tx * stamp_at(st, x1, y1, g, G);
        val = (1.f - ty) * top + ty * bot;
        if ((double)val < gmin) val = 0.f;
    }
    out[id] = val;
}

}  // namespace

extern "C" int vpho_frame_patch_f32(const unsigned char* frames, int n, int H, int W, const double* minv, const float* colour, const unsigned char* flip,
                                    const int* erase, const unsigned int* key, int P, float* out, void* stream) {
    VPHO_REQUIRE(n >= 0 && H > 0 && W > 0 && P > 0 && P <= 16384, "vpho_frame_patch_f32: bad size (n %d, H %d, W %d, P %d)", n, H, W, P);
    if (n == 0) return 0;
    VPHO_REQUIRE(frames && minv && out && n <= 65535, "vpho_frame_patch_f32: NULL frames / minv / out, or more than 65535 frames");
    VPHO_REQUIRE(!erase || key, "vpho_frame_patch_f32: erase rectangles without a Philox key");
    VPHO_REQUIRE((long long)H * W * 3 < (1ll << 40), "vpho_frame_patch_f32: frame too large");
    const PatchArgs a{frames, minv, colour, flip, erase, key, out, H, W, P};
    const long long blocks = ((long long)P * P + 255) / 256;
    hipLaunchKernelGGL(frame_patch_kernel, dim3((unsigned)blocks, (unsigned)n), dim3(256), 0, (hipStream_t)stream, a);
    return vpho::check_launch("frame_patch_kernel");
}

extern "C" int vpho_heatmap_targets_f32(const double* pts, const double* box, const int* res, const unsigned char* left, const float* g, int G, double sigma,
                                        double gmin, int n, int J, int S, int adaptive, float* out, void* stream) {
    VPHO_REQUIRE(n >= 0 && J > 0 && S > 0 && S <= 4096 && G > 0 && G <= 4096 && sigma > 0.0, "vpho_heatmap_targets_f32: bad size (n %d, J %d, S %d, G %d)", n, J, S, G);
    if (n == 0) return 0;
    VPHO_REQUIRE(pts && box && g && out && (!adaptive || res), "vpho_heatmap_targets_f32: NULL argument");
    const long long total = (long long)n * J * S * S;
    const long long blocks = (total + 255) / 256;
    VPHO_REQUIRE(blocks < (1ll << 31), "vpho_heatmap_targets_f32: too many output cells");
    hipLaunchKernelGGL(heatmap_targets_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, pts, box, res, left, g, G, sigma, gmin, J, S, adaptive, out, total);
    return vpho::check_launch("heatmap_targets_kernel");
}
