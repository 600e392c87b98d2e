// The photometric augmentations of the reference's ImageAugmentor (lib/dataset/base.py:349-397) that need a per-image statistic or a
// neighbourhood, on the device: A.CLAHE, the contrast and hue of A.ColorJitter, A.AdvancedBlur and A.MotionBlur.  The rules are this
// project's own restatement: every stage ends on an integer grey level, so the image between two stages is uint8.
//   photo_levels_kernel      the bicubic crop of frame_patch_kernel (frames.hip), stored as levels (n,P,P,3) uint8
//   photo_clahe_lut_kernel   one workgroup per (sample, tile): L8 of the tile, 256-bin histogram in LDS, clip, redistribute, LUT
//   photo_clahe_apply_kernel bilinear interpolation between four LUTs in integers, back through Lab
//   photo_grey_sum_kernel    integer sum of the grey levels after shift and brightness (the mean of the contrast stage)
//   photo_colour_kernel      shift, brightness, contrast, saturation, hue
//   photo_filter_kernel      two K x K filters (K <= 7) with reflect-101 borders from LDS tiles, mirror, normalisation, erasing
// Integer atomics only (LDS histogram, one 64-bit add per workgroup for the grey sum): nothing depends on the order of workgroups.
// Every index into a frame, a plane, a LUT, an LDS tile and the output is checked.
// The bicubic crop, level(), the normalisation and the erasing are frames.hip's own code (frames_common.h).
#include "common.h"
#include "frames_common.h"
#include "../../include/vpho_hip.h"
#include <cstdint>

namespace {

__device__ __forceinline__ float level64(double v) { return (float)fmin(fmax(rint(v), 0.0), 255.0); }

// ---------------------------------------------------------------------------------------------------------------- levels
__global__ __launch_bounds__(256) void photo_levels_kernel(const unsigned char* __restrict__ frames, const double* __restrict__ minv,
                                                           unsigned char* __restrict__ out, int H, int W, int P) {
    const int s = blockIdx.y;
    const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
    if (pix >= (long long)P * P) return;
    const int y = (int)(pix / P), x = (int)(pix % P);
    float v[3];
    bicubic_crop(frames + (long long)s * H * W * 3, H, W, minv + 6 * (long long)s, x, y, v);
    unsigned char* q = out + ((long long)s * P * P + pix) * 3;
    q[0] = (unsigned char)v[0];
    q[1] = (unsigned char)v[1];
    q[2] = (unsigned char)v[2];
}

// ---------------------------------------------------------------------------------------------------------------- Lab (fp64)
// sRGB (IEC 61966-2-1) <-> CIE Lab, D65, white (0.950456, 1, 1.088754): the constants of OpenCV's floating-point path
__device__ __forceinline__ double lab_f(double t) { return t > 0.008856 ? cbrt(t) : 7.787 * t + 16.0 / 116.0; }
__device__ __forceinline__ double lab_finv(double f) {
    const double c = f * f * f;
    return c > 0.008856 ? c : (f - 16.0 / 116.0) / 7.787;
}
__device__ __forceinline__ double srgb_to_linear(double c) { return c <= 0.04045 ? c / 12.92 : pow((c + 0.055) / 1.055, 2.4); }
__device__ __forceinline__ double linear_to_srgb(double c) { return c <= 0.0031308 ? 12.92 * c : 1.055 * pow(c, 1.0 / 2.4) - 0.055; }
// lin: the 256 linearised levels (LDS).  Returns f(X / Xn), f(Y), f(Z / Zn)
__device__ __forceinline__ void rgb_to_fxyz(const double* lin, const unsigned char* p, double& fX, double& fY, double& fZ) {
    const double r = lin[p[0]], g = lin[p[1]], b = lin[p[2]];
    const double X = (0.412453 * r + 0.357580 * g) + 0.180423 * b;
    const double Y = (0.212671 * r + 0.715160 * g) + 0.072169 * b;
    const double Z = (0.019334 * r + 0.119193 * g) + 0.950227 * b;
    fX = lab_f(X / 0.950456);
    fY = lab_f(Y);
    fZ = lab_f(Z / 1.088754);
}
__device__ __forceinline__ int l8_of(double fY) {
    const double L = 116.0 * fY - 16.0;
    return (int)fmin(fmax(rint(L * 255.0 / 100.0), 0.0), 255.0);
}

// ---------------------------------------------------------------------------------------------------------------- CLAHE
// grid (64, n): tile blockIdx.x of sample blockIdx.y.  clip[s] == 0: the sample's gate is off, nothing is written for it.
__global__ __launch_bounds__(256) void photo_clahe_lut_kernel(const unsigned char* __restrict__ levels, const int* __restrict__ clip,
                                                              unsigned char* __restrict__ l8, unsigned char* __restrict__ lut, int P) {
    __shared__ double lin[256];
    __shared__ unsigned int hist[256];
    __shared__ unsigned int scan[2][256];
    __shared__ unsigned int excess;
    const int s = blockIdx.y, tile = blockIdx.x, t = threadIdx.x;
    const int cl = clip[s];
    if (cl <= 0) return;                                                         // uniform over the workgroup
    const int tw = P / 8, ty0 = (tile / 8) * tw, tx0 = (tile % 8) * tw, area = tw * tw;
    lin[t] = srgb_to_linear((double)t / 255.0);
    hist[t] = 0u;
    if (t == 0) excess = 0u;
    __syncthreads();
    for (int i = t; i < area; i += 256) {
        const int y = ty0 + i / tw, x = tx0 + i % tw;                            // < P: the tile lies inside the plane
        const long long at = (long long)s * P * P + (long long)y * P + x;
        double fX, fY, fZ;
        rgb_to_fxyz(lin, levels + at * 3, fX, fY, fZ);
        const int v = l8_of(fY);
        l8[at] = (unsigned char)v;
        atomicAdd(&hist[v], 1u);
    }
    __syncthreads();
    unsigned int h = hist[t];
    if (h > (unsigned)cl) {
        atomicAdd(&excess, h - (unsigned)cl);
        h = (unsigned)cl;
    }
    __syncthreads();
    const unsigned int ex = excess, batch = ex / 256u, resid = ex - batch * 256u;
    h += batch;
    if (resid > 0u) {
        const unsigned int step = max(256u / resid, 1u);                         // bins 0, step, 2 step, ... take one count each
        if ((unsigned)t % step == 0u && (unsigned)t / step < resid) h += 1u;
    }
    int cur = 0;
    scan[0][t] = h;
    __syncthreads();
#pragma unroll
    for (int d = 1; d < 256; d <<= 1) {                                          // inclusive sum over the bins
        scan[cur ^ 1][t] = scan[cur][t] + (t >= d ? scan[cur][t - d] : 0u);
        cur ^= 1;
        __syncthreads();
    }
    const unsigned long long num = 255ull * scan[cur][t];
    unsigned long long q = num / (unsigned)area;
    const unsigned long long r = num - q * (unsigned)area;
    if (2 * r > (unsigned)area || (2 * r == (unsigned)area && (q & 1ull))) q += 1;   // round half to even
    lut[((long long)s * 64 + tile) * 256 + t] = (unsigned char)(q > 255ull ? 255ull : q);
}

// one thread per pixel.  out may be levels (each thread reads and writes its own pixel only); l8_out (n,P,P) may be NULL.
__global__ __launch_bounds__(256) void photo_clahe_apply_kernel(const unsigned char* levels, const int* __restrict__ clip, const unsigned char* __restrict__ l8,
                                                                const unsigned char* __restrict__ lut, unsigned char* out, unsigned char* l8_out, int P) {
    __shared__ double lin[256];
    const int s = blockIdx.y;
    const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool on = clip[s] > 0;
    if (on) lin[threadIdx.x] = srgb_to_linear((double)threadIdx.x / 255.0);
    __syncthreads();
    if (pix >= (long long)P * P) return;
    const long long at = (long long)s * P * P + pix;
    const unsigned char* p = levels + at * 3;
    unsigned char* q = out + at * 3;
    if (!on) {                                                                   // no Lab round trip
        const unsigned char r = p[0], g = p[1], b = p[2];
        q[0] = r; q[1] = g; q[2] = b;
        return;
    }
    const int y = (int)(pix / P), x = (int)(pix % P), tw = P / 8;
    // tile coordinate (2 x + 1 - tw) / (2 tw): floor and remainder in integers
    const int ax = 2 * x + 1 - tw, ay = 2 * y + 1 - tw;
    const int fx = ax >= 0 ? ax / (2 * tw) : -1, fy = ay >= 0 ? ay / (2 * tw) : -1;      // ax >= -tw + 1 > -2 tw
    const int xa = ax - fx * 2 * tw, ya = ay - fy * 2 * tw;                      // in [0, 2 tw)
    const int tx1 = min(max(fx, 0), 7), tx2 = min(max(fx + 1, 0), 7), ty1 = min(max(fy, 0), 7), ty2 = min(max(fy + 1, 0), 7);
    const int v = l8[at];
    const unsigned char* base = lut + (long long)s * 64 * 256 + v;
    const long long l11 = base[(ty1 * 8 + tx1) * 256], l12 = base[(ty1 * 8 + tx2) * 256], l21 = base[(ty2 * 8 + tx1) * 256], l22 = base[(ty2 * 8 + tx2) * 256];
    const long long xb = 2 * tw - xa, yb = 2 * tw - ya, den = 4ll * tw * tw;
    const long long num = (xb * yb * l11 + xa * yb * l12) + (xb * ya * l21 + (long long)xa * ya * l22);
    long long o = num / den;
    const long long r = num - o * den;
    if (2 * r > den || (2 * r == den && (o & 1ll))) o += 1;
    if (l8_out) l8_out[at] = (unsigned char)o;
    double fX, fY, fZ;
    rgb_to_fxyz(lin, p, fX, fY, fZ);
    const double a = 500.0 * (fX - fY), b = 200.0 * (fY - fZ);                   // a and b stay unquantised
    const double L = (double)o * 100.0 / 255.0;
    const double gY = (L + 16.0) / 116.0, gX = gY + a / 500.0, gZ = gY - b / 200.0;
    const double X = lab_finv(gX) * 0.950456, Y = lab_finv(gY), Z = lab_finv(gZ) * 1.088754;
    const double R = (3.240479 * X + -1.53715 * Y) + -0.498535 * Z;
    const double G = (-0.969256 * X + 1.875991 * Y) + 0.041556 * Z;
    const double B = (0.055648 * X + -0.204043 * Y) + 1.057311 * Z;
    q[0] = (unsigned char)level64(255.0 * linear_to_srgb(R));
    q[1] = (unsigned char)level64(255.0 * linear_to_srgb(G));
    q[2] = (unsigned char)level64(255.0 * linear_to_srgb(B));
}

// ---------------------------------------------------------------------------------------------------------------- colour
// shift and brightness as frame_patch_kernel has them; c = the sample's five numbers or NULL
__device__ __forceinline__ void shift_brightness(const float* c, float* v) {
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = level(v[k] + c[k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = level(v[k] * c[3]);
}
__device__ __forceinline__ float grey_of(const float* v) { return level((0.299f * v[0] + 0.587f * v[1]) + 0.114f * v[2]); }

// sums (n) unsigned 64-bit, zero on entry.  1024 pixels per workgroup: LDS integer add, then one 64-bit add per workgroup.
__global__ __launch_bounds__(256) void photo_grey_sum_kernel(const unsigned char* __restrict__ levels, const float* __restrict__ colour,
                                                             unsigned long long* __restrict__ sums, int P) {
    __shared__ unsigned int part;
    const int s = blockIdx.y;
    if (threadIdx.x == 0) part = 0u;
    __syncthreads();
    unsigned int mine = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long pix = (long long)blockIdx.x * 1024 + j * 256 + threadIdx.x;
        if (pix < (long long)P * P) {
            const unsigned char* p = levels + ((long long)s * P * P + pix) * 3;
            float v[3] = {(float)p[0], (float)p[1], (float)p[2]};
            if (colour) shift_brightness(colour + 5 * (long long)s, v);
            mine += (unsigned int)grey_of(v);
        }
    }
    atomicAdd(&part, mine);
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(sums + s, (unsigned long long)part);
}

// torchvision's _rgb2hsv / _hsv2rgb in fp32 on v / 255, h + delta - floor(h + delta) between them; every operation rounded once
__device__ __forceinline__ void hue_shift(float* v, float delta) {
    const float r = v[0] / 255.0f, g = v[1] / 255.0f, b = v[2] / 255.0f;
    const float maxc = fmaxf(fmaxf(r, g), b), minc = fminf(fminf(r, g), b);
    const bool eq = maxc == minc;
    const float cr = maxc - minc;
    const float sat = cr / (eq ? 1.0f : maxc);
    const float div = eq ? 1.0f : cr;
    const float rc = (maxc - r) / div, gc = (maxc - g) / div, bc = (maxc - b) / div;
    float h = maxc == r ? bc - gc : (maxc == g ? (2.0f + rc) - bc : (4.0f + gc) - rc);
    h = fmodf(h / 6.0f + 1.0f, 1.0f);
    const float hs = h + delta;
    h = hs - floorf(hs);
    const float h6 = h * 6.0f, fl = floorf(h6), f = h6 - fl;
    const int i = ((int)fl % 6 + 6) % 6;
    const float one = 1.0f;
    const float p = fminf(fmaxf(maxc * (one - sat), 0.f), 1.f);
    const float q = fminf(fmaxf(maxc * (one - sat * f), 0.f), 1.f);
    const float t = fminf(fmaxf(maxc * (one - sat * (one - f)), 0.f), 1.f);
    const float R = i == 0 || i == 5 ? maxc : (i == 1 ? q : (i == 4 ? t : p));
    const float G = i == 1 || i == 2 ? maxc : (i == 0 ? t : (i == 3 ? q : p));
    const float B = i == 3 || i == 4 ? maxc : (i == 2 ? t : (i == 5 ? q : p));
    v[0] = level(R * 255.0f);
    v[1] = level(G * 255.0f);
    v[2] = level(B * 255.0f);
}

// out may be levels.  colour (n,5), contrast (n), hue (n) may each be NULL; sums (n) is read only where contrast is given.
__global__ __launch_bounds__(256) void photo_colour_kernel(const unsigned char* levels, const float* __restrict__ colour, const float* __restrict__ contrast,
                                                           const float* __restrict__ hue, const unsigned long long* __restrict__ sums, unsigned char* out, int P) {
    const int s = blockIdx.y;
    const long long pix = (long long)blockIdx.x * 256 + threadIdx.x, N = (long long)P * P;
    if (pix >= N) return;
    const unsigned char* p = levels + ((long long)s * N + pix) * 3;
    float v[3] = {(float)p[0], (float)p[1], (float)p[2]};
    const float* c = colour ? colour + 5 * (long long)s : nullptr;
    if (c) shift_brightness(c, v);
    if (contrast) {
        const float f = contrast[s];
        const float m = (float)((2ull * sums[s] + (unsigned long long)N) / (2ull * (unsigned long long)N));   // the integer mean, <= 255
        const float g1 = (1.f - f) * m;
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = level(f * v[k] + g1);
    }
    if (c) {
        const float sat = c[4];
        const float g1 = (1.f - sat) * grey_of(v);
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = level(sat * v[k] + g1);
    }
    if (hue) {
        const float d = hue[s];
        if (d != 0.f) hue_shift(v, d);
    }
    unsigned char* q = out + ((long long)s * N + pix) * 3;
    q[0] = (unsigned char)v[0];
    q[1] = (unsigned char)v[1];
    q[2] = (unsigned char)v[2];
}

// ---------------------------------------------------------------------------------------------------------------- filters + finish
constexpr int FT = 32;                       // output tile, FT x FT pixels, 256 threads
constexpr int FA = FT + 12;                  // input tile: 6-pixel halo (two filters of up to 7 x 7)
constexpr int FB = FT + 6;                   // intermediate tile: 3-pixel halo
// BORDER_REFLECT_101 for any i and any n >= 1: ... 2 1 | 0 1 2 ... n-1 | n-2 n-3 ...
__device__ __forceinline__ int reflect101(int i, int n) {
    if (n == 1) return 0;
    const int period = 2 * (n - 1);
    i %= period;
    if (i < 0) i += period;
    return i < n ? i : period - i;
}

struct FilterArgs {
    const unsigned char* levels; const float* k1; const int* K1; const float* k2; const int* K2;
    const unsigned char* flip; const int* erase; const unsigned int* key; float* out; int P;
};

__global__ __launch_bounds__(256) void photo_filter_kernel(const FilterArgs a) {
    __shared__ uint32_t A[FA * FA];              // a pixel per word, r | g << 8 | b << 16: one LDS read per tap
    __shared__ uint32_t B[FB * FB];
    __shared__ float w1[49], w2[49];
    const int P = a.P, s = blockIdx.z, t = threadIdx.x;
    const int x0 = blockIdx.x * FT, y0 = blockIdx.y * FT;
    const int x1 = min(x0 + FT, P), y1 = min(y0 + FT, P);                        // the tile's pixels: [x0, x1) x [y0, y1)
    int Ka = a.K1[s], Kb = a.K2[s];
    const bool bad = Ka < 1 || Ka > 7 || !(Ka & 1) || Kb < 1 || Kb > 7 || !(Kb & 1);   // the caller refuses these; a bad size reads nothing and gives NaN
    if (bad) Ka = Kb = 1;
    if (t < 49) {
        w1[t] = t < Ka * Ka ? a.k1[49 * (long long)s + t] : 0.f;
        w2[t] = t < Kb * Kb ? a.k2[49 * (long long)s + t] : 0.f;
    }
    const unsigned char* img = a.levels + (long long)s * P * P * 3;
    for (int i = t; i < FA * FA; i += 256) {                                     // input at virtual coordinates, reflected into the image
        const int yy = reflect101(y0 - 6 + i / FA, P), xx = reflect101(x0 - 6 + i % FA, P);
        const unsigned char* p = img + ((long long)yy * P + xx) * 3;
        A[i] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    }
    __syncthreads();
    // first filter at the tile + 3: a position outside the image holds the intermediate image at its reflection, that is the filter
    // CENTRED at the reflected position (not the filter of reflected taps, which differs for a kernel that is not symmetric)
    const int ha = Ka / 2, hb = Kb / 2;
    for (int i = t; i < FB * FB; i += 256) {
        const int vy = y0 - 3 + i / FB, vx = x0 - 3 + i % FB;
        float acc[3] = {0.f, 0.f, 0.f};
        if (vx < x1 + 3 && vy < y1 + 3) {
            const int ax = reflect101(vx, P) - ha - (x0 - 6), ay = reflect101(vy, P) - ha - (y0 - 6);
            if (ax >= 0 && ay >= 0 && ax + Ka <= FA && ay + Ka <= FA) {
                for (int ky = 0; ky < Ka; ++ky)
                    for (int kx = 0; kx < Ka; ++kx) {
                        const float w = w1[ky * Ka + kx];
                        const uint32_t p = A[(ay + ky) * FA + ax + kx];
                        acc[0] += w * (float)(p & 255u);
                        acc[1] += w * (float)((p >> 8) & 255u);
                        acc[2] += w * (float)((p >> 16) & 255u);
                    }
            }
        }
        B[i] = (uint32_t)level(acc[0]) | ((uint32_t)level(acc[1]) << 8) | ((uint32_t)level(acc[2]) << 16);
    }
    __syncthreads();
    const bool flip = a.flip && a.flip[s];
    const int lx = t % FT, x = x0 + lx;
#pragma unroll
    for (int j = 0; j < FT / 8; ++j) {
        const int ly = t / FT + 8 * j, y = y0 + ly;
        if (x >= P || y >= P) continue;
        float v[3] = {0.f, 0.f, 0.f};
        const int bx = lx + 3 - hb, by = ly + 3 - hb;                            // >= 0, and bx + Kb <= lx + 7 <= FB
        for (int ky = 0; ky < Kb; ++ky)
            for (int kx = 0; kx < Kb; ++kx) {
                const float w = w2[ky * Kb + kx];
                const uint32_t p = B[(by + ky) * FB + bx + kx];
                v[0] += w * (float)(p & 255u);
                v[1] += w * (float)((p >> 8) & 255u);
                v[2] += w * (float)((p >> 16) & 255u);
            }
        v[0] = level(v[0]); v[1] = level(v[1]); v[2] = level(v[2]);
        // from here on as frame_patch_kernel: the patch column x lands at xo, erasing is in output coordinates
        const int xo = flip ? P - 1 - x : x;
        const long long pix = (long long)y * P + xo;
        float o[3];
        normalise_erase(v, a.erase, a.key, s, xo, y, pix, o);
        if (bad) o[0] = o[1] = o[2] = __builtin_nanf("");
        float* q = a.out + (long long)s * 3 * P * P + pix;
        q[0] = o[0];
        q[(long long)P * P] = o[1];
        q[2ll * P * P] = o[2];
    }
}

bool photo_sizes_ok(int n, int P) { return n >= 0 && n <= 65535 && P > 0 && P <= 16384; }

}  // namespace

extern "C" int vpho_photo_levels_u8(const unsigned char* frames, int n, int H, int W, const double* minv, int P, unsigned char* out, void* stream) {
    VPHO_REQUIRE(photo_sizes_ok(n, P) && H > 0 && W > 0, "vpho_photo_levels_u8: bad size (n %d, H %d, W %d, P %d)", n, H, W, P);
    if (n == 0) return 0;
    VPHO_REQUIRE(frames && minv && out, "vpho_photo_levels_u8: NULL frames / minv / out");
    VPHO_REQUIRE((long long)H * W * 3 < (1ll << 40), "vpho_photo_levels_u8: frame too large");
    const long long blocks = ((long long)P * P + 255) / 256;
    hipLaunchKernelGGL(photo_levels_kernel, dim3((unsigned)blocks, (unsigned)n), dim3(256), 0, (hipStream_t)stream, frames, minv, out, H, W, P);
    return vpho::check_launch("photo_levels_kernel");
}

extern "C" int vpho_photo_clahe_lut_u8(const unsigned char* levels, const int* clip, int n, int P, unsigned char* l8, unsigned char* lut, void* stream) {
    VPHO_REQUIRE(photo_sizes_ok(n, P) && P % 8 == 0, "vpho_photo_clahe_lut_u8: bad size (n %d, P %d): the 8 x 8 tile grid needs P %% 8 == 0", n, P);
    if (n == 0) return 0;
    VPHO_REQUIRE(levels && clip && l8 && lut, "vpho_photo_clahe_lut_u8: NULL argument");
    hipLaunchKernelGGL(photo_clahe_lut_kernel, dim3(64, (unsigned)n), dim3(256), 0, (hipStream_t)stream, levels, clip, l8, lut, P);
    return vpho::check_launch("photo_clahe_lut_kernel");
}

extern "C" int vpho_photo_clahe_apply_u8(const unsigned char* levels, const int* clip, const unsigned char* l8, const unsigned char* lut, int n, int P,
                                         unsigned char* out, unsigned char* l8_out, void* stream) {
    VPHO_REQUIRE(photo_sizes_ok(n, P) && P % 8 == 0, "vpho_photo_clahe_apply_u8: bad size (n %d, P %d): the 8 x 8 tile grid needs P %% 8 == 0", n, P);
    if (n == 0) return 0;
    VPHO_REQUIRE(levels && clip && l8 && lut && out, "vpho_photo_clahe_apply_u8: NULL argument");
    const long long blocks = ((long long)P * P + 255) / 256;
    hipLaunchKernelGGL(photo_clahe_apply_kernel, dim3((unsigned)blocks, (unsigned)n), dim3(256), 0, (hipStream_t)stream, levels, clip, l8, lut, out, l8_out, P);
    return vpho::check_launch("photo_clahe_apply_kernel");
}

extern "C" int vpho_photo_grey_sum_u8(const unsigned char* levels, const float* colour, int n, int P, long long* sums, void* stream) {
    VPHO_REQUIRE(photo_sizes_ok(n, P), "vpho_photo_grey_sum_u8: bad size (n %d, P %d)", n, P);
    if (n == 0) return 0;
    VPHO_REQUIRE(levels && sums, "vpho_photo_grey_sum_u8: NULL levels / sums");
    const long long blocks = ((long long)P * P + 1023) / 1024;
    hipLaunchKernelGGL(photo_grey_sum_kernel, dim3((unsigned)blocks, (unsigned)n), dim3(256), 0, (hipStream_t)stream, levels, colour,
                       reinterpret_cast<unsigned long long*>(sums), P);
    return vpho::check_launch("photo_grey_sum_kernel");
}

extern "C" int vpho_photo_colour_u8(const unsigned char* levels, const float* colour, const float* contrast, const float* hue, const long long* sums, int n,
                                    int P, unsigned char* out, void* stream) {
    VPHO_REQUIRE(photo_sizes_ok(n, P), "vpho_photo_colour_u8: bad size (n %d, P %d)", n, P);
    if (n == 0) return 0;
    VPHO_REQUIRE(levels && out, "vpho_photo_colour_u8: NULL levels / out");
    VPHO_REQUIRE(!contrast || sums, "vpho_photo_colour_u8: contrast factors without the grey sums");
    const long long blocks = ((long long)P * P + 255) / 256;
    hipLaunchKernelGGL(photo_colour_kernel, dim3((unsigned)blocks, (unsigned)n), dim3(256), 0, (hipStream_t)stream, levels, colour, contrast, hue,
                       reinterpret_cast<const unsigned long long*>(sums), out, P);
    return vpho::check_launch("photo_colour_kernel");
}

extern "C" int vpho_photo_filter_f32(const unsigned char* levels, const float* k1, const int* K1, const float* k2, const int* K2, const unsigned char* flip,
                                     const int* erase, const unsigned int* key, int n, int P, float* out, void* stream) {
    VPHO_REQUIRE(photo_sizes_ok(n, P), "vpho_photo_filter_f32: bad size (n %d, P %d)", n, P);
    if (n == 0) return 0;
    VPHO_REQUIRE(levels && k1 && K1 && k2 && K2 && out, "vpho_photo_filter_f32: NULL argument");
    VPHO_REQUIRE(!erase || key, "vpho_photo_filter_f32: erase rectangles without a Philox key");
    const FilterArgs a{levels, k1, K1, k2, K2, flip, erase, key, out, P};
    const unsigned tiles = (unsigned)((P + FT - 1) / FT);
    hipLaunchKernelGGL(photo_filter_kernel, dim3(tiles, tiles, (unsigned)n), dim3(256), 0, (hipStream_t)stream, a);
    return vpho::check_launch("photo_filter_kernel");
}
