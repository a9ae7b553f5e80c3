#pragma once
// of3d_solve.hpp — the pointwise 3x3 solve and the smallest eigenvalue (pipeline overview:
// of3d_common.hpp).
#include "of3d_common.hpp"

namespace {

// ---------------------------------------------------------------------------
// Solves.  Expression trees copied from calc_flow.py:337-340 (3D) and
// :154-168 (2D); numpy's x**-1 is a correctly rounded reciprocal, x**2 = x*x.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void solve3(double x2, double y2, double z2, double xy, double xz, double yz, double tx,
                                       double ty, double tz, double& vx, double& vy, double& vz) {
    double det = x2 * y2 * z2;
    det = det + 2.0 * xy * xz * yz;
    det = det - y2 * (xz * xz);
    det = det - z2 * (xy * xy);
    det = det - x2 * (yz * yz);
    const double nR = -(1.0 / (det + kEps));
    vx = nR * ((y2 * z2 - yz * yz) * tx + (xz * yz - xy * z2) * ty + (xy * yz - xz * y2) * tz);
    vy = nR * ((yz * xz - xy * z2) * tx + (x2 * z2 - xz * xz) * ty + (xz * xy - x2 * yz) * tz);
    vz = nR * ((xy * yz - y2 * xz) * tx + (xy * xz - x2 * yz) * ty + (x2 * y2 - xy * xy) * tz);
}

// cos((2/3) acos(u)) for u in [0, 1]: a degree-16 polynomial in t = 2u - 1 (Chebyshev fit,
// monomial coefficients in t, |coef| <= 0.77: Horner is stable), max error 1.4e-15 — analytic on
// [0, 1] (the acos branch points at u = +-1 cancel in the even cosine at u = 1; u = -1 is outside).
// Coefficients from tools/eig_poly.py.  Replaces the library acos and a cos series (~110 VALU
// instructions per voxel, a third of K5c's solve tail) by 16 FMAs.
// one Horner step c * t + k with k in an SGPR pair (written out: the compiler's own choice, a
// v_fmac_f64 with k moved into VGPRs first, costs two v_mov per coefficient and voxel)
__device__ __forceinline__ double fma_sk(double c, double t, double k) {
    double d;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(d) : "v"(c), "v"(t), "s"(k));
    return d;
}
__device__ __forceinline__ double cos_two_thirds_acos(double u) {
    const double t = 2.0 * u - 1.0;
    double c = fma_sk(-1.627207239089953e-10, t, 5.267127096337474e-10);
    c = fma_sk(c, t, -1.0560891259645176e-09);
    c = fma_sk(c, t, 3.6015719568912613e-09);
    c = fma_sk(c, t, -1.3476196916010413e-08);
    c = fma_sk(c, t, 4.617990510403794e-08);
    c = fma_sk(c, t, -1.594699400417876e-07);
    c = fma_sk(c, t, 5.639770165191962e-07);
    c = fma_sk(c, t, -2.035894233312921e-06);
    c = fma_sk(c, t, 7.541131934033293e-06);
    c = fma_sk(c, t, -2.8919931795498364e-05);
    c = fma_sk(c, t, 0.00011642544430647587);
    c = fma_sk(c, t, -0.0005041246915259092);
    c = fma_sk(c, t, 0.0024663528157121257);
    c = fma_sk(c, t, -0.015509188436476284);
    c = fma_sk(c, t, 0.2474090663228402);
    return fma_sk(c, t, 0.7660444431189779);
}

// Smallest eigenvalue of the symmetric 3x3 [[a d e][d b f][e f c]] in fp64
// (trigonometric closed form).  The reference gets it from LAPACK cgeev in
// complex64 (calc_flow.py:355-357); fp64 here, stored as float32 like the
// reference's output (or kept fp64 with OF3D_REL_F64).
// lambda_min = q + 2p cos(phi + 2pi/3) = q - 2p cos(pi/3 - phi), phi = acos(r)/3 in [0, pi/3];
// pi/3 - acos(r)/3 = (2/3) acos(u) with u = sqrt((1 - r) / 2) (acos(-r) = 2 acos(u)), so
// lambda_min = q - 2p cos((2/3) acos(u)): one polynomial, no acos / cos.  Same conditioning as
// the acos form: near r = 1 (the two SMALLEST eigenvalues nearly equal: flat / isotropic or
// rank-1 regions) r's rounding reaches u through a square root, an error of ~sqrt(eps) p —
// tools/eig_poly.py measures 1.7e-8 lambda_max there.  That is far inside the float32 rel's
// 1e-6 lambda_max, but not the fp64 rel's 1e-10 (OF3D_REL_F64, MATLAB's pageeig,
// M/calc_flow3D.m:235-236), so the fp64-rel instances (REFINE) take eigmin3_deflate below for
// w = (1 - r) / 2 < 1e-6: there lambda_max is simple and far from the pair, so its eigenvector
// is well conditioned, and the pair's smaller eigenvalue comes from the 2x2 block on the plane
// orthogonal to it with the cancellation-free 2x2 formula (max 1e-13 lambda_max over
// tools/eig_poly.py's near-degenerate, isotropic and rank-1 sets; tests/test_eig_formula.py).
// The branch is taken by whole waves only where such tensors occur; float32-rel instances
// never compile it.
// It works on the scaled matrix B = (T - qI) / p (entries O(1), the caller's B11 .. B23), so the
// cross products' squared norms neither underflow nor overflow whatever the tensor's magnitude
// (unscaled, entries below ~1e-77 or above ~1e77 gave NaN); the caller multiplies by p.
__device__ __forceinline__ double eigmin3_deflate(double aq, double bq, double cq, double d, double e, double f,
                                               double w) {
    // B's largest eigenvalue 2 cos(phi) with phi = (2/3) asin(u): cos(phi) = 1 - (2/9) w + O(w^2)
    // (an error in mu only tilts the eigenvector, which moves the 2x2 block's eigenvalues at
    // second order)
    const double mu = 2.0 * (1.0 - (2.0 / 9.0) * w);
    const double m00 = aq - mu, m11 = bq - mu, m22 = cq - mu;
    // the eigenvector of mu: the longest cross product of two rows of E - mu I (rank 2)
    const double c0x = d * f - e * m11, c0y = e * d - m00 * f, c0z = m00 * m11 - d * d;
    const double c1x = d * m22 - e * f, c1y = e * e - m00 * m22, c1z = m00 * f - d * e;
    const double c2x = m11 * m22 - f * f, c2y = f * e - d * m22, c2z = d * f - m11 * e;
    const double n0 = c0x * c0x + c0y * c0y + c0z * c0z, n1 = c1x * c1x + c1y * c1y + c1z * c1z,
                 n2 = c2x * c2x + c2y * c2y + c2z * c2z;
    double vx = c0x, vy = c0y, vz = c0z, nn = n0;
    if (n1 > nn) vx = c1x, vy = c1y, vz = c1z, nn = n1;
    if (n2 > nn) vx = c2x, vy = c2y, vz = c2z, nn = n2;
    const double iv = 1.0 / sqrt(nn);
    vx *= iv, vy *= iv, vz *= iv;
    // an orthonormal basis (u1, u2) of the plane orthogonal to v
    double ux, uy, uz;
    if (fabs(vx) > fabs(vy)) {
        const double s = 1.0 / sqrt(vx * vx + vz * vz);
        ux = -vz * s, uy = 0.0, uz = vx * s;
    } else {
        const double s = 1.0 / sqrt(vy * vy + vz * vz);
        ux = 0.0, uy = vz * s, uz = -vy * s;
    }
    const double wx = vy * uz - vz * uy, wy = vz * ux - vx * uz, wz = vx * uy - vy * ux;
    // the 2x2 block [[al ga][ga be]] of E on that plane
    const double e1x = aq * ux + d * uy + e * uz, e1y = d * ux + bq * uy + f * uz, e1z = e * ux + f * uy + cq * uz;
    const double e2x = aq * wx + d * wy + e * wz, e2y = d * wx + bq * wy + f * wz, e2z = e * wx + f * wy + cq * wz;
    const double al = ux * e1x + uy * e1y + uz * e1z;
    const double be = wx * e2x + wy * e2y + wz * e2z;
    const double ga = ux * e2x + uy * e2y + uz * e2z;
    const double h = (al - be) * 0.5;
    return (al + be) * 0.5 - sqrt(h * h + ga * ga);
}

template <bool REFINE = false>
__device__ __forceinline__ double eigmin3(double a, double b, double c, double d, double e, double f) {
    const double p1 = d * d + e * e + f * f;
    if (p1 == 0.0) return fmin(a, fmin(b, c));
    // constant divisions as multiplications by the rounded reciprocal (not bit-matched
    // anyway; an IEEE division is a ~10-instruction sequence)
    constexpr double third = 1.0 / 3.0, sixth = 1.0 / 6.0;
    const double q = (a + b + c) * third;
    const double aq = a - q, bq = b - q, cq = c - q;
    const double p2 = aq * aq + bq * bq + cq * cq + 2.0 * p1;
    // p = sqrt(x) and 1 / p from one reciprocal square root (v_rsq_f64 + 2 Newton steps: ~1e-16
    // relative; the IEEE sqrt and division sequences cost twice the instructions); tensors
    // too small for the hardware estimate take the IEEE path (p1 > 0, so x > 0)
    const double x = p2 * sixth;
    double p, ip;
    if (x > 1e-290 && x < 1e290) {
        ip = __builtin_amdgcn_rsq(x);
        ip = ip * (1.5 - 0.5 * x * ip * ip);
        ip = ip * (1.5 - 0.5 * x * ip * ip);
        p = x * ip;
    } else {
        p = sqrt(x);
        ip = 1.0 / p;
    }
    const double B11 = aq * ip, B22 = bq * ip, B33 = cq * ip, B12 = d * ip, B13 = e * ip, B23 = f * ip;
    const double detB =
        B11 * (B22 * B33 - B23 * B23) - B12 * (B12 * B33 - B23 * B13) + B13 * (B12 * B23 - B22 * B13);
    double r = 0.5 * detB;
    r = fmin(1.0, fmax(-1.0, r));
    // u = sqrt(w), w in [0, 1], the same way (w floored at 1e-290: u < 1e-145 reads as 0)
    const double w = fmax((1.0 - r) * 0.5, 1e-290);
    if constexpr (REFINE) {
        if (w < 1e-6) return q + p * eigmin3_deflate(B11, B22, B33, B12, B13, B23, w);
    }
    double iu = __builtin_amdgcn_rsq(w);
    iu = iu * (1.5 - 0.5 * w * iu * iu);
    iu = iu * (1.5 - 0.5 * w * iu * iu);
    return q - 2.0 * p * cos_two_thirds_acos(w * iu);
}

// eigmin3 for G tensors at once, straight-line: the per-tensor branches of eigmin3 become
// per-lane selects, and its rare paths (tensors too small / large for the rsq estimate; the
// fp64-rel deflation) wave-uniform branches taken only when some lane of the wave needs them.
// Every tensor goes through exactly eigmin3<REFINE>'s operations (bit-identical), but as G
// independent chains the scheduler can interleave: K5c's epilogue ran one dependent chain per
// voxel (IEEE divisions, rsq Newton steps, the polynomial) with two waves per SIMD to hide it.
template <bool REFINE, int G>
__device__ __forceinline__ void eigmin3_group(const double (&a)[G], const double (&b)[G], const double (&c)[G],
                                              const double (&d)[G], const double (&e)[G], const double (&f)[G],
                                              double (&out)[G]) {
    constexpr double third = 1.0 / 3.0, sixth = 1.0 / 6.0;
    double q[G], aq[G], bq[G], cq[G], x[G], p[G], ip[G];
    bool diag[G], slow[G], any_slow = false;
#pragma unroll
    for (int i = 0; i < G; ++i) {
        const double p1 = d[i] * d[i] + e[i] * e[i] + f[i] * f[i];
        diag[i] = p1 == 0.0;
        q[i] = (a[i] + b[i] + c[i]) * third;
        aq[i] = a[i] - q[i], bq[i] = b[i] - q[i], cq[i] = c[i] - q[i];
        const double p2 = aq[i] * aq[i] + bq[i] * bq[i] + cq[i] * cq[i] + 2.0 * p1;
        x[i] = p2 * sixth;
        double r = __builtin_amdgcn_rsq(x[i]);
        r = r * (1.5 - 0.5 * x[i] * r * r);
        r = r * (1.5 - 0.5 * x[i] * r * r);
        ip[i] = r;
        p[i] = x[i] * r;
        slow[i] = !diag[i] && !(x[i] > 1e-290 && x[i] < 1e290);
        any_slow |= slow[i];
    }
    if (__builtin_expect(__any(any_slow), 0)) {  // IEEE sqrt / division where rsq cannot serve
#pragma unroll
        for (int i = 0; i < G; ++i)
            if (slow[i]) {
                p[i] = sqrt(x[i]);
                ip[i] = 1.0 / p[i];
            }
    }
    double B11[G], B22[G], B33[G], B12[G], B13[G], B23[G], w[G];
    bool defl[G], any_defl = false;
#pragma unroll
    for (int i = 0; i < G; ++i) {
        B11[i] = aq[i] * ip[i], B22[i] = bq[i] * ip[i], B33[i] = cq[i] * ip[i];
        B12[i] = d[i] * ip[i], B13[i] = e[i] * ip[i], B23[i] = f[i] * ip[i];
        const double detB = B11[i] * (B22[i] * B33[i] - B23[i] * B23[i]) - B12[i] * (B12[i] * B33[i] - B23[i] * B13[i]) +
                            B13[i] * (B12[i] * B23[i] - B22[i] * B13[i]);
        double r = 0.5 * detB;
        r = fmin(1.0, fmax(-1.0, r));
        w[i] = fmax((1.0 - r) * 0.5, 1e-290);
        defl[i] = REFINE && !diag[i] && w[i] < 1e-6;
        any_defl |= defl[i];
        double iu = __builtin_amdgcn_rsq(w[i]);
        iu = iu * (1.5 - 0.5 * w[i] * iu * iu);
        iu = iu * (1.5 - 0.5 * w[i] * iu * iu);
        out[i] = q[i] - 2.0 * p[i] * cos_two_thirds_acos(w[i] * iu);
    }
    if constexpr (REFINE) {
        if (__builtin_expect(__any(any_defl), 0)) {
#pragma unroll
            for (int i = 0; i < G; ++i)
                if (defl[i]) out[i] = q[i] + p[i] * eigmin3_deflate(B11[i], B22[i], B33[i], B12[i], B13[i], B23[i], w[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < G; ++i)
        if (diag[i]) out[i] = fmin(a[i], fmin(b[i], c[i]));
}

}  // namespace
