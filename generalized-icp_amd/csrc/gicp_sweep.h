// gicp_sweep.h — motion compensation of a sweep: the per-point map, shared by the device
// kernel (gicp_sweep.hip) and the host entry points (gicp_capi.cpp), and the kernel's arguments.
//
// A sweep is a cloud p_i with one stamp tau_i per point, a motion M = P(tau)^-1 P(tau + 1) and a reference
// stamp ref.  With xi = Log(M) = (omega, v) the de-skewed point is p'_i = Exp((tau_i - ref) xi) p_i; with
// s = tau_i - ref, phi = s omega, u = s v, theta = |phi| and phi^ the cross-product matrix of phi
//   p' = R(phi) p + V(phi) u,   R = I + A phi^ + B phi^2,   V = I + B phi^ + C phi^2,
//   A = sin(theta) / theta,  B = (1 - cos(theta)) / theta^2,  C = (theta - sin(theta)) / theta^3
// (Rodrigues' formula and its integral over the stamp).  In 2-D phi is a scalar and phi^ = phi J, J = (0 -1; 1 0).
#pragma once
#include <stdint.h>

#include <cmath>

#ifndef __host__
#define __host__
#define __device__
#endif

namespace gicp {

// A, B, C of the angle theta >= 0 given as t2 = theta^2.  Below theta = 0.1 their Taylor series to theta^8
// (the next term is below 2^-63 of the first): the closed forms cancel there -- (1 - cos(theta)) / theta^2 in
// floating point is 0 at theta = 1e-8, not 1/2.  Above it B comes from the half angle (no cancellation), and
// theta - sin(theta) has lost at most 13 bits, which its factor theta^2 |u| / 6 pays back.
__host__ __device__ inline void sweep_coeffs(double t2, double& A, double& B, double& C) {
    if (t2 < 1e-2) {
        A = 1.0 + t2 * (-1.0 / 6.0 + t2 * (1.0 / 120.0 + t2 * (-1.0 / 5040.0 + t2 * (1.0 / 362880.0))));
        B = 0.5 + t2 * (-1.0 / 24.0 + t2 * (1.0 / 720.0 + t2 * (-1.0 / 40320.0 + t2 * (1.0 / 3628800.0))));
        C = 1.0 / 6.0 + t2 * (-1.0 / 120.0 + t2 * (1.0 / 5040.0 + t2 * (-1.0 / 362880.0 + t2 * (1.0 / 39916800.0))));
    } else {
        const double t = sqrt(t2), sn = sin(t), sh = sin(0.5 * t);
        A = sn / t;
        B = 2.0 * sh * sh / t2;
        C = (t - sn) / (t2 * t);
    }
}

// The per-point map: p' = Exp(s xi) p, s = stamp - ref.  xi = (omega[3], v[3]) in 3-D, (omega, v[2]) in 2-D.
// s = 0 and xi = 0 return p (every correction term is then an exact zero).
template <int D>
__host__ __device__ inline void sweep_point(const double* xi, double s, const double* p, double* out) {
    double A, B, C;
    if constexpr (D == 3) {
        const double f0 = s * xi[0], f1 = s * xi[1], f2 = s * xi[2];
        const double u0 = s * xi[3], u1 = s * xi[4], u2 = s * xi[5];
        sweep_coeffs(f0 * f0 + f1 * f1 + f2 * f2, A, B, C);
        // phi x p, phi x (phi x p) and the same of u
        const double c0 = f1 * p[2] - f2 * p[1], c1 = f2 * p[0] - f0 * p[2], c2 = f0 * p[1] - f1 * p[0];
        const double d0 = f1 * c2 - f2 * c1, d1 = f2 * c0 - f0 * c2, d2 = f0 * c1 - f1 * c0;
        const double e0 = f1 * u2 - f2 * u1, e1 = f2 * u0 - f0 * u2, e2 = f0 * u1 - f1 * u0;
        const double g0 = f1 * e2 - f2 * e1, g1 = f2 * e0 - f0 * e2, g2 = f0 * e1 - f1 * e0;
        out[0] = p[0] + ((A * c0 + B * d0) + (u0 + (B * e0 + C * g0)));
        out[1] = p[1] + ((A * c1 + B * d1) + (u1 + (B * e1 + C * g1)));
        out[2] = p[2] + ((A * c2 + B * d2) + (u2 + (B * e2 + C * g2)));
    } else {
        const double f = s * xi[0], u0 = s * xi[1], u1 = s * xi[2];
        const double f2 = f * f;
        sweep_coeffs(f2, A, B, C);
        // phi^ p = f (-y, x), phi^2 p = -f^2 p
        const double Af = A * f, Bf = B * f, Bf2 = B * f2, Cf2 = C * f2;
        out[0] = p[0] + ((-Af * p[1] - Bf2 * p[0]) + (u0 + (-Bf * u1 - Cf2 * u0)));
        out[1] = p[1] + ((Af * p[0] - Bf2 * p[1]) + (u1 + (Bf * u0 - Cf2 * u1)));
    }
}

// k_deskew (gicp_sweep.hip): pts [n][dim] is de-skewed in place; res takes the voxel filter's first six result
// words (gicp_internal.h kVoxelRes): the ordered-integer min[3] and max[3] of the de-skewed points.
struct SweepArgs {
    double* pts;
    const double* stamps;     // [n]
    int64_t n;
    int32_t dim;
    double xi[6];             // the twist (dim 2: three values)
    double ref;
    unsigned long long* res;
};

}  // namespace gicp
