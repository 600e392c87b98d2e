// The data front end on the device: what the reference's Dataset.__getitem__ does per image on CPU workers, as two launches per batch.
//   frame_patch_kernel      lib/dataset/dexycb6.py:345 (cv2.warpAffine, INTER_CUBIC, constant border 0), :389-391 (RGBShift, brightness and
//                           saturation of ColorJitter), :398-399 (left hands mirrored), :442-444 (normalize_rgb, timm RandomErasing 'pixel')
//   heatmap_targets_kernel  lib/utils/misc_fn.py:285-385 (HeatmapGenerator.get_heatmap, AdaptiveHeatmapGenerator.__call__)
// Both are one thread per output pixel, no LDS, no atomics; every index into the frame, the Gaussian table and the output is checked.
#include "common.h"
#include "../../include/vpho_hip.h"
#include <cstdint>

namespace {

// ---------------------------------------------------------------------------------------------------------------- Philox4x32-10
struct U4 { uint32_t x, y, z, w; };
__device__ __forceinline__ U4 philox4x32_10(U4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c.x, p1 = (uint64_t)0xCD9E8D57u * c.z;
        c = U4{(uint32_t)(p1 >> 32) ^ c.y ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c.w ^ k1, (uint32_t)p0};
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}
// a word's upper 23 bits as u = (k + 0.5) / 2^23 in (0, 1): exact in fp32, never 0 or 1
__device__ __forceinline__ float unit23(uint32_t w) { return ((float)(w >> 9) + 0.5f) * (1.0f / 8388608.0f); }
// Box-Muller: r = sqrt(-2 ln u1), (r cos 2 pi u2, r sin 2 pi u2); |value| <= sqrt(2 * 24 ln 2) = 5.77
__device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, float& z0, float& z1) {
    const float r = sqrtf(-2.0f * logf(unit23(a)));
    float s, c;
    sincospif(2.0f * unit23(b), &s, &c);
    z0 = r * c;
    z1 = r * s;
}

// ---------------------------------------------------------------------------------------------------------------- warp + colour
// Keys' cubic convolution weights with A = -0.75 for the taps at floor - 1 .. floor + 2 (OpenCV's interpolateCubic)
__device__ __forceinline__ void cubic_weights(float t, float* w) {
    const float A = -0.75f;
    w[0] = ((A * (t + 1.f) - 5.f * A) * (t + 1.f) + 8.f * A) * (t + 1.f) - 4.f * A;
    w[1] = ((A + 2.f) * t - (A + 3.f)) * t * t + 1.f;
    w[2] = ((A + 2.f) * (1.f - t) - (A + 3.f)) * (1.f - t) * (1.f - t) + 1.f;
    w[3] = 1.f - w[0] - w[1] - w[2];
}
__device__ __forceinline__ float level(float v) { return fminf(fmaxf(rintf(v), 0.f), 255.f); }      // a NaN becomes 0

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
    const double* m = a.minv + 6 * (long long)s;
    const double sx = m[0] * xs + m[1] * y + m[2], sy = m[3] * xs + m[4] * y + m[5];
    float v[3] = {0.f, 0.f, 0.f};
    // a coordinate that leaves every tap outside the frame (or is not finite) gives the border value 0
    if (sx > -3.0 && sx < (double)a.W + 2.0 && sy > -3.0 && sy < (double)a.H + 2.0) {
        const double fx = floor(sx), fy = floor(sy);
        const int ix = (int)fx, iy = (int)fy;
        float wx[4], wy[4];
        cubic_weights((float)(sx - fx), wx);
        cubic_weights((float)(sy - fy), wy);
        const unsigned char* f = a.frames + (long long)s * a.H * a.W * 3;
        float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int yy = iy - 1 + j;
            float row[3] = {0.f, 0.f, 0.f};
            if (yy >= 0 && yy < a.H) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int xx = ix - 1 + i;
                    if (xx >= 0 && xx < a.W) {
                        const unsigned char* p = f + ((long long)yy * a.W + xx) * 3;
                        row[0] += wx[i] * (float)p[0];
                        row[1] += wx[i] * (float)p[1];
                        row[2] += wx[i] * (float)p[2];
                    }
                }
            }
            acc[0] += wy[j] * row[0];
            acc[1] += wy[j] * row[1];
            acc[2] += wy[j] * row[2];
        }
        v[0] = level(acc[0]); v[1] = level(acc[1]); v[2] = level(acc[2]);
    }
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
    const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
    float o[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = (v[k] / 255.0f - mean[k]) / sd[k];
    if (a.erase) {
        const int* e = a.erase + 16 * (long long)s;
        bool in = false;
#pragma unroll
        for (int r = 0; r < 4; ++r) in = in || (x >= e[4 * r] && x < e[4 * r + 2] && y >= e[4 * r + 1] && y < e[4 * r + 3]);
        if (in) {
            const U4 w = philox4x32_10(U4{(uint32_t)pix, 0u, 0u, 0u}, a.key[2 * s], a.key[2 * s + 1]);
            float z3;
            box_muller(w.x, w.y, o[0], o[1]);
            box_muller(w.z, w.w, o[2], z3);
        }
    }
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
