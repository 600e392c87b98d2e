// The double-sigmoid contact weight of detect_hand_and_object_contact (lib/utils/physics_fn.py:47-117), shared by contact.hip (the label
// chain) and contact_multi.hip (every sampled hypothesis): one definition, so both weigh a normal distance with the same bits.
#pragma once

namespace {

__device__ inline double contact_weight(double x, double mid1, double mid2) {
    const double m1 = 1.0 + exp(-1600.0 * (x - mid1));
    const double m2 = 1.0 + exp(1600.0 * (x - mid2));
    if (!isfinite(m1) || !isfinite(m2)) return 0.0;
    return 1.0 / (m1 * m2 + 1e-10);
}

}  // namespace
