// Device code that frames.hip (frame_patch_kernel) and photo.hip (photo_levels_kernel, photo_filter_kernel) share: the counter-based
// random numbers of the erased pixels, the bicubic crop of a frame and the end of a patch (normalisation, erasing).  One copy, so the
// photometric path and the plain path produce the same bits where their rules are the same (tests/test_gpu_photo.py compares them).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

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

// ---------------------------------------------------------------------------------------------------------------- bicubic crop
// Keys' cubic convolution weights with A = -0.75 for the taps at floor - 1 .. floor + 2 (OpenCV's interpolateCubic)
__device__ __forceinline__ void cubic_weights(float t, float* w) {
    const float A = -0.75f;
    w[0] = ((A * (t + 1.f) - 5.f * A) * (t + 1.f) + 8.f * A) * (t + 1.f) - 4.f * A;
    w[1] = ((A + 2.f) * t - (A + 3.f)) * t * t + 1.f;
    w[2] = ((A + 2.f) * (1.f - t) - (A + 3.f)) * (1.f - t) * (1.f - t) + 1.f;
    w[3] = 1.f - w[0] - w[1] - w[2];
}
__device__ __forceinline__ float level(float v) { return fminf(fmaxf(rintf(v), 0.f), 255.f); }      // a NaN becomes 0

// cv2.warpAffine(INTER_CUBIC, constant border 0) at the patch pixel (column x, row y): frame (H,W,3) uint8 of one sample, m its six minv
// numbers -> v, three integer grey levels.  Rows outside the frame are skipped, each row's taps summed first, then the rows.
__device__ __forceinline__ void bicubic_crop(const unsigned char* frame, int H, int W, const double* m, int x, int y, float* v) {
    const double sx = m[0] * x + m[1] * y + m[2], sy = m[3] * x + m[4] * y + m[5];
    v[0] = v[1] = v[2] = 0.f;
    // a coordinate that leaves every tap outside the frame (or is not finite) gives the border value 0
    if (sx > -3.0 && sx < (double)W + 2.0 && sy > -3.0 && sy < (double)H + 2.0) {
        const double fx = floor(sx), fy = floor(sy);
        const int ix = (int)fx, iy = (int)fy;
        float wx[4], wy[4];
        cubic_weights((float)(sx - fx), wx);
        cubic_weights((float)(sy - fy), wy);
        float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int yy = iy - 1 + j;
            float row[3] = {0.f, 0.f, 0.f};
            if (yy >= 0 && yy < H) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int xx = ix - 1 + i;
                    if (xx >= 0 && xx < W) {
                        const unsigned char* p = frame + ((long long)yy * W + xx) * 3;
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
}

// ---------------------------------------------------------------------------------------------------------------- the end of a patch
// normalize_rgb and timm's RandomErasing 'pixel' at the OUTPUT pixel (x, y), pix = y * P + x, of sample s: levels v -> o.  erase (n,16):
// four rectangles a sample, or NULL; key (n,2): the samples' Philox words, read only inside a rectangle.
__device__ __forceinline__ void normalise_erase(const float* v, const int* erase, const unsigned int* key, int s, int x, int y, long long pix, float* o) {
    const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = (v[k] / 255.0f - mean[k]) / sd[k];
    if (erase) {
        const int* e = erase + 16 * (long long)s;
        bool in = false;
#pragma unroll
        for (int r = 0; r < 4; ++r) in = in || (x >= e[4 * r] && x < e[4 * r + 2] && y >= e[4 * r + 1] && y < e[4 * r + 3]);
        if (in) {
            const U4 w = philox4x32_10(U4{(uint32_t)pix, 0u, 0u, 0u}, key[2 * s], key[2 * s + 1]);
            float z3;
            box_muller(w.x, w.y, o[0], o[1]);
            box_muller(w.z, w.w, o[2], z3);
        }
    }
}
