/* vpho_photo.h -- C ABI of libvpho_photo.so, the photometric augmentation of the training crops (vpho_amd/csrc/photo.hip).
 *
 * A library of its own beside libvpho_hip.so: the ABI of include/vpho_hip.h is closed at its 128 entry points (its tests compare the
 * header, the documents and `nm -D` with that number), and nothing on the inference path needs what is here.  The conventions are those
 * of vpho_hip.h: every function returns 0 on success and non-zero on failure, with the text of the failure in vpho_photo_last_error()
 * (this library's own slot); device pointers in, the HIP stream last; the functions below are the library's ONLY exported symbols
 * (tests/test_photo_cpu.py compares `nm -D` with this header).
 */
#ifndef VPHO_PHOTO_H
#define VPHO_PHOTO_H

#if defined(__GNUC__) || defined(__clang__)
#define VPHO_PHOTO_API __attribute__((visibility("default")))
#else
#define VPHO_PHOTO_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

VPHO_PHOTO_API const char* vpho_photo_last_error(void);
/* ---- photometric augmentation (photo.hip): the transforms of the reference's ImageAugmentor
 * (lib/dataset/base.py:349-397) that need a per-image statistic or a neighbourhood -- A.CLAHE, the contrast and hue of A.ColorJitter,
 * A.AdvancedBlur, A.MotionBlur -- as this project's own rules (no parity with albumentations or OpenCV is claimed).
 * Every stage ends on an integer grey level: the image between two stages is `levels` (n,P,P,3) uint8.  n <= 65535, P <= 16384; n == 0:
 * success without a launch.  Stages in the reference's order, on the UNMIRRORED patch: levels, CLAHE, colour, filter (which mirrors last).
 * vpho_photo_levels_u8: the bicubic crop of vpho_frame_patch_f32 (same minv, same arithmetic) before any colour stage, not mirrored.
 * vpho_photo_clahe_lut_u8 (P % 8 == 0, an 8 x 8 grid of tiles of tw = P / 8 pixels a side): clip (n) int32, 0 = the sample's gate is off
 * (nothing is written for it), else the clip count max(1, int(clip_limit * tw * tw / 256)) formed by the caller.  l8 (n,P,P): rint(L * 255
 * / 100) of CIE Lab in fp64 (sRGB linearisation 0.04045 / 12.92 / 2.4, the D65 matrix, white (0.950456, 1, 1.088754), f(t) = cbrt(t) above
 * 0.008856, else 7.787 t + 16 / 116).  lut (n,64,256), tile ty * 8 + tx, integers only: the tile's histogram of l8, counts above clip cut
 * off, excess / 256 added to every bin, the remaining r counts given one each to bins 0, step, 2 step, ... (step = max(256 / r, 1)),
 * lut[i] = 255 * cumsum[i] / (tw * tw) rounded half to even.
 * vpho_photo_clahe_apply_u8: per pixel the four LUTs around the tile coordinate (2 x + 1 - tw) / (2 tw) (tile indices clamped to 0..7),
 * bilinear as an integer numerator over 4 tw tw, rounded half to even -> l8_out (n,P,P; may be NULL); L' = l8' * 100 / 255 with the
 * pixel's own unquantised a and b back to sRGB in fp64, rounded and clamped -> out (may be levels).  A sample with clip 0 is copied.
 * vpho_photo_grey_sum_u8: sums (n) 64-bit, ZERO on entry: the sum over the image of gray = round(0.299 R + 0.587 G + 0.114 B) after the
 * shift and brightness of colour (n,5; NULL: of the levels as they are).  Integer adds only: the same bits in every run.
 * vpho_photo_colour_u8: v + d, v * b (colour, as vpho_frame_patch_f32), contrast (n) or NULL: f * v + (1 - f) * m with the integer mean
 * m = (2 sum + N) / (2 N), N = P * P, of sums; saturation (colour); hue (n) or NULL, 0 = skipped: v / 255 to HSV by torchvision's formulas,
 * h + delta - floor(h + delta), back, times 255.  All fp32, every operation rounded once, every stage rounded and clamped.  out may be levels.
 * vpho_photo_filter_f32: two filters, then the mirror, normalisation and erasing of vpho_frame_patch_f32 (flip, erase, key as there) ->
 * out (n,3,P,P) fp32.  k1, k2 (n,49) fp32: a K x K kernel, row-major, in the first K * K entries, K1, K2 (n) int32 odd in 1..7 (anything
 * else gives that sample NaN; the caller refuses it).  Each filter is the correlation sum_ky sum_kx k[ky][kx] * v[y + ky - K/2][x + kx -
 * K/2], accumulated in fp32 from 0 in that order, border reflect-101, rounded and clamped; the second reads the first's integer image. */
VPHO_PHOTO_API int vpho_photo_levels_u8(const unsigned char* frames, int n, int H, int W, const double* minv, int P, unsigned char* out, void* stream);
VPHO_PHOTO_API int vpho_photo_clahe_lut_u8(const unsigned char* levels, const int* clip, int n, int P, unsigned char* l8, unsigned char* lut, void* stream);
VPHO_PHOTO_API int vpho_photo_clahe_apply_u8(const unsigned char* levels, const int* clip, const unsigned char* l8, const unsigned char* lut, int n, int P,
                              unsigned char* out, unsigned char* l8_out, void* stream);
VPHO_PHOTO_API int vpho_photo_grey_sum_u8(const unsigned char* levels, const float* colour, int n, int P, long long* sums, void* stream);
VPHO_PHOTO_API int vpho_photo_colour_u8(const unsigned char* levels, const float* colour, const float* contrast, const float* hue, const long long* sums, int n,
                         int P, unsigned char* out, void* stream);
VPHO_PHOTO_API int vpho_photo_filter_f32(const unsigned char* levels, const float* k1, const int* K1, const float* k2, const int* K2, const unsigned char* flip,
                          const int* erase, const unsigned int* key, int n, int P, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
