// The per-triangle record of the penetration kernels (include/vpho_hip.h) and the exact point-triangle distance both of them use:
// penetration.hip (every triangle) and penetration_multi.hip (the triangles its bounds cannot reject) call the same tri_dist2 on the
// same record fields and the same p, so their distances have the same bits.
#pragma once
#include "../../include/vpho_hip.h"

namespace {

static_assert(VPHO_PEN_TRI_STRIDE == 28, "record layout below");

// record fields (include/vpho_hip.h)
enum { R_CX = 0, R_CY, R_A00, R_A01, R_A10, R_A11, R_SDET, R_ADET, R_T1X, R_T1Y, R_N0, R_N1, R_SNZ, R_ANZ, R_D0,
       R_CX0, R_CX1, R_CY0, R_CY1, R_AX, R_AY, R_AZ, R_ABX, R_ABY, R_ABZ, R_ACX, R_ACY, R_ACZ };

__device__ inline double dot3(double ax, double ay, double az, double bx, double by, double bz) { return ax * bx + ay * by + az * bz; }

// squared distance from p to the triangle (a, a + ab, a + ac), g = fields R_AX .. R_ACZ of its record; ap = p - a
__device__ inline double tri_dist2_geo(const double* g, double px, double py, double pz) {
    const double abx = g[3], aby = g[4], abz = g[5], acx = g[6], acy = g[7], acz = g[8];
    const double apx = px - g[0], apy = py - g[1], apz = pz - g[2];
    const double d1 = dot3(abx, aby, abz, apx, apy, apz), d2 = dot3(acx, acy, acz, apx, apy, apz);
    if (d1 <= 0.0 && d2 <= 0.0) return dot3(apx, apy, apz, apx, apy, apz);                                   // vertex a
    const double bpx = apx - abx, bpy = apy - aby, bpz = apz - abz;
    const double d3 = dot3(abx, aby, abz, bpx, bpy, bpz), d4 = dot3(acx, acy, acz, bpx, bpy, bpz);
    if (d3 >= 0.0 && d4 <= d3) return dot3(bpx, bpy, bpz, bpx, bpy, bpz);                                     // vertex b
    const double vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {                                                                // edge ab
        const double s = d1 / (d1 - d3);
        const double ex = apx - s * abx, ey = apy - s * aby, ez = apz - s * abz;
        return dot3(ex, ey, ez, ex, ey, ez);
    }
    const double cpx = apx - acx, cpy = apy - acy, cpz = apz - acz;
    const double d5 = dot3(abx, aby, abz, cpx, cpy, cpz), d6 = dot3(acx, acy, acz, cpx, cpy, cpz);
    if (d6 >= 0.0 && d5 <= d6) return dot3(cpx, cpy, cpz, cpx, cpy, cpz);                                     // vertex c
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {                                                                // edge ac
        const double s = d2 / (d2 - d6);
        const double ex = apx - s * acx, ey = apy - s * acy, ez = apz - s * acz;
        return dot3(ex, ey, ez, ex, ey, ez);
    }
    const double va = d3 * d6 - d5 * d4;
    if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {                                                  // edge bc
        const double s = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        const double ex = bpx - s * (acx - abx), ey = bpy - s * (acy - aby), ez = bpz - s * (acz - abz);
        return dot3(ex, ey, ez, ex, ey, ez);
    }
    const double den = va + vb + vc;
    if (!(den > 0.0)) {                                   // zero-area triangle: nearest of its corners (its edges belong to other faces)
        const double a2 = dot3(apx, apy, apz, apx, apy, apz), b2 = dot3(bpx, bpy, bpz, bpx, bpy, bpz), c2 = dot3(cpx, cpy, cpz, cpx, cpy, cpz);
        return fmin(a2, fmin(b2, c2));
    }
    const double v = vb / den, w = vc / den;                                                                  // face interior
    const double ex = apx - v * abx - w * acx, ey = apy - v * aby - w * acy, ez = apz - v * abz - w * acz;
    return dot3(ex, ey, ez, ex, ey, ez);
}

static_assert(R_ACZ - R_AX == 8 && R_ACZ == VPHO_PEN_TRI_STRIDE - 1, "tri_dist2_geo reads the last nine fields");
__device__ inline double tri_dist2(const double* r, double px, double py, double pz) { return tri_dist2_geo(r + R_AX, px, py, pz); }

}  // namespace
