// The per-triangle record of the penetration kernels (include/vpho_hip.h) and the exact point-triangle distance both of them use:
// penetration.hip (every triangle) and penetration_multi.hip (the triangles its bounds cannot reject) call the same tri_dist2 on the
// same record fields and the same p, so their distances have the same bits.  The pose transform p = R^T (v - t), the hash frame, the
// point's hash cell and one triangle's step of the z-ray parity rule live here too: the two penetration kernels and the intersection
// volume (intersection_volume.hip, whose records hold fields 0-18 only) call the same functions, so their inside flags have the same bits.
#pragma once
#include "../../include/vpho_hip.h"

namespace {

static_assert(VPHO_PEN_TRI_STRIDE == 28, "record layout below");

// record fields (include/vpho_hip.h)
enum { R_CX = 0, R_CY, R_A00, R_A01, R_A10, R_A11, R_SDET, R_ADET, R_T1X, R_T1Y, R_N0, R_N1, R_SNZ, R_ANZ, R_D0,
       R_CX0, R_CX1, R_CY0, R_CY1, R_AX, R_AY, R_AZ, R_ABX, R_ABY, R_ABZ, R_ACX, R_ACY, R_ACZ };

__device__ inline double dot3(double ax, double ay, double az, double bx, double by, double bz) { return ax * bx + ay * by + az * bz; }

// p = R^T (v - t) in the model frame: R = [R | t] (3, 4) row-major fp64, v an fp32 camera-frame point
__device__ inline void pen_model_frame(const double* R, const float* v, double& px, double& py, double& pz) {
    const double d0 = (double)v[0] - R[3], d1 = (double)v[1] - R[7], d2 = (double)v[2] - R[11];
    px = R[0] * d0 + R[4] * d1 + R[8] * d2;
    py = R[1] * d0 + R[5] * d1 + R[9] * d2;
    pz = R[2] * d0 + R[6] * d1 + R[10] * d2;
}

// q = scale * p + translate in the hash frame
__device__ inline void pen_hash_frame(const double* sc, const double* tr, double px, double py, double pz, double& qx, double& qy, double& qz) {
    qx = sc[0] * px + tr[0];
    qy = sc[1] * py + tr[1];
    qz = sc[2] * pz + tr[2];
}

// cull to [0, 512]^3 and the point's own hash cell (q >= 0 there: truncation == floor); a point on the far faces (q == 512) has no
// cell and no triangle.  -> has a cell; cx = cy = -1 outside the box
__device__ inline bool pen_cell(double qx, double qy, double qz, double& cx, double& cy) {
    const double res = (double)VPHO_PEN_RESOLUTION;
    const bool in_box = 0.0 <= qx && qx <= res && 0.0 <= qy && qy <= res && 0.0 <= qz && qz <= res;
    cx = in_box ? (double)(int)qx : -1.0;
    cy = in_box ? (double)(int)qy : -1.0;
    return in_box && cx < res && cy < res;
}

// one triangle of the z-ray parity rule, r = its record (fields 0-18 are read): cell test, strict containment, the two depth buckets
__device__ inline void pen_parity_step(const double* r, double qx, double qy, double qz, double cx, double cy, unsigned& par0, unsigned& par1) {
    if (r[R_CX0] <= cx && cx <= r[R_CX1] && r[R_CY0] <= cy && cy <= r[R_CY1]) {
        // strict 2-D containment (check_triangles): y = q - t3, (u, v) by the adjugate, scaled by sign(det A)
        const double y0 = qx - r[R_CX], y1 = qy - r[R_CY];
        const double sdet = r[R_SDET], adet = r[R_ADET];
        const double u = (r[R_A11] * y0 - r[R_A01] * y1) * sdet;
        const double w = (-r[R_A10] * y0 + r[R_A00] * y1) * sdet;
        const double suv = u + w;
        if (0.0 < u && u < adet && 0.0 < w && w < adet && 0.0 < suv && suv < adet) {
            // plane depth against q_z |n_z| (compute_intersection_depth); D0 = t1_z |n_z|, NaN where n_z == 0
            const double alpha = r[R_N0] * (r[R_T1X] - qx) + r[R_N1] * (r[R_T1Y] - qy);
            const double depth = r[R_D0] + alpha * r[R_SNZ];
            const double zz = qz * r[R_ANZ];
            par0 ^= (depth >= zz) ? 1u : 0u;
            par1 ^= (depth < zz) ? 1u : 0u;
        }
    }
}

// pen_parity_step split at the point where q_z first enters, for callers whose points share q_x, q_y and the cell (the centres of one
// lattice column, intersection_volume_multi.hip): the same operations on the same operands in the same order, so
//   if (pen_parity_xy(r, qx, qy, cx, cy, depth)) pen_parity_z(r, depth, qz, par0, par1);
// leaves in par0, par1 the bits pen_parity_step(r, qx, qy, qz, cx, cy, par0, par1) leaves.  -> the triangle's projection holds (qx, qy)
__device__ inline bool pen_parity_xy(const double* r, double qx, double qy, double cx, double cy, double& depth) {
    if (r[R_CX0] <= cx && cx <= r[R_CX1] && r[R_CY0] <= cy && cy <= r[R_CY1]) {
        const double y0 = qx - r[R_CX], y1 = qy - r[R_CY];
        const double sdet = r[R_SDET], adet = r[R_ADET];
        const double u = (r[R_A11] * y0 - r[R_A01] * y1) * sdet;
        const double w = (-r[R_A10] * y0 + r[R_A00] * y1) * sdet;
        const double suv = u + w;
        if (0.0 < u && u < adet && 0.0 < w && w < adet && 0.0 < suv && suv < adet) {
            const double alpha = r[R_N0] * (r[R_T1X] - qx) + r[R_N1] * (r[R_T1Y] - qy);
            depth = r[R_D0] + alpha * r[R_SNZ];
            return true;
        }
    }
    return false;
}

__device__ inline void pen_parity_z(const double* r, double depth, double qz, unsigned& par0, unsigned& par1) {
    const double zz = qz * r[R_ANZ];
    par0 ^= (depth >= zz) ? 1u : 0u;
    par1 ^= (depth < zz) ? 1u : 0u;
}

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

__device__ inline double pen_sign(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : (x == 0.0 ? 0.0 : x)); }      // numpy.sign

// fields 0-18 of the record of one triangle from its corners t[corner][axis] in the hash frame, in the order of operations of
// vpho_amd/physics_eval.py mesh_tables (which builds the object meshes' records on the host): for a mesh that changes per launch
__device__ inline void pen_face_record(const double (*t)[3], double* r) {
    const double res1 = (double)(VPHO_PEN_RESOLUTION - 1);
    // A = (t1 - t3, t2 - t3) as columns, det A
    const double A00 = t[0][0] - t[2][0], A01 = t[1][0] - t[2][0], A10 = t[0][1] - t[2][1], A11 = t[1][1] - t[2][1];
    const double det = A00 * A11 - A01 * A10;
    // n = (t3 - t1) x (t2 - t1), numpy.cross: a product, a product, their difference
    const double ux = t[2][0] - t[0][0], uy = t[2][1] - t[0][1], uz = t[2][2] - t[0][2];
    const double wx = t[1][0] - t[0][0], wy = t[1][1] - t[0][1], wz = t[1][2] - t[0][2];
    const double n0 = uy * wz - uz * wy, n1 = uz * wx - ux * wz, n2 = ux * wy - uy * wx;
    const double an2 = fabs(n2);
    r[R_CX] = t[2][0]; r[R_CY] = t[2][1];
    r[R_A00] = A00; r[R_A01] = A01; r[R_A10] = A10; r[R_A11] = A11;
    r[R_SDET] = pen_sign(det); r[R_ADET] = fabs(det);
    r[R_T1X] = t[0][0]; r[R_T1Y] = t[0][1];
    r[R_N0] = n0; r[R_N1] = n1;
    r[R_SNZ] = pen_sign(n2); r[R_ANZ] = an2;
    r[R_D0] = an2 != 0.0 ? t[0][2] * an2 : NAN;
    // the triangle hash's cells: int-truncated bbox of the xy projection, clamped to [0, RESOLUTION)
    r[R_CX0] = fmin(fmax(trunc(fmin(fmin(t[0][0], t[1][0]), t[2][0])), 0.0), res1);
    r[R_CX1] = fmin(fmax(trunc(fmax(fmax(t[0][0], t[1][0]), t[2][0])), 0.0), res1);
    r[R_CY0] = fmin(fmax(trunc(fmin(fmin(t[0][1], t[1][1]), t[2][1])), 0.0), res1);
    r[R_CY1] = fmin(fmax(trunc(fmax(fmax(t[0][1], t[1][1]), t[2][1])), 0.0), res1);
}

static_assert(R_ACZ - R_AX == 8 && R_ACZ == VPHO_PEN_TRI_STRIDE - 1, "tri_dist2_geo reads the last nine fields");
__device__ inline double tri_dist2(const double* r, double px, double py, double pz) { return tri_dist2_geo(r + R_AX, px, py, pz); }

}  // namespace
