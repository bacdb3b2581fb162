// The least-squares fit shared by th_superpose (superpose.hip) and th_tmscore (tmscore.hip): the finiteness test of a position, one
// Jacobi rotation and Horn's quaternion route from a 3 x 3 cross-covariance to the proper rotation; the wave-wide sums are
// device_math.h's.  Device code for one 64-lane wavefront; every lane computes the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include "device_math.h"

// every float64 product and sum below is rounded separately, as the NumPy restatement's are
#pragma clang fp contract(off)

namespace {

constexpr int kWave = 64;
constexpr int kSweeps = 10;                       // Jacobi sweeps at most (a 4 x 4 matrix is diagonal to the last bit after 5 or 6)

__device__ inline bool finite3(double x, double y, double z) { return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z); }

// one Jacobi rotation in the (P, Q) plane: A <- J^T A J, V <- V J
template <int P, int Q>
__device__ inline void rotate(double (&A)[4][4], double (&V)[4][4]) {
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    const double root = fabs(theta) + sqrt(theta * theta + 1.0);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / root;
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double akp = A[k][P], akq = A[k][Q];
        A[k][P] = c * akp - s * akq;
        A[k][Q] = s * akp + c * akq;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double apk = A[P][k], aqk = A[Q][k];
        A[P][k] = c * apk - s * aqk;
        A[Q][k] = s * apk + c * aqk;
    }
    A[P][Q] = 0.0;
    A[Q][P] = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double vkp = V[k][P], vkq = V[k][Q];
        V[k][P] = c * vkp - s * vkq;
        V[k][Q] = s * vkp + c * vkq;
    }
}

// the proper rotation (row-major R[9]) that takes the centred mobile coordinates onto the centred reference ones, from the
// cross-covariance S[x][y] = sum mob_x ref_y: the unit eigenvector of largest eigenvalue of Horn's matrix is its quaternion
__device__ inline void horn_rotation(const double (&S)[3][3], double (&R)[9]) {
    double A[4][4], V[4][4];
    A[0][0] = (S[0][0] + S[1][1]) + S[2][2];
    A[1][1] = (S[0][0] - S[1][1]) - S[2][2];
    A[2][2] = (S[1][1] - S[0][0]) - S[2][2];
    A[3][3] = (S[2][2] - S[0][0]) - S[1][1];
    A[0][1] = A[1][0] = S[1][2] - S[2][1];
    A[0][2] = A[2][0] = S[2][0] - S[0][2];
    A[0][3] = A[3][0] = S[0][1] - S[1][0];
    A[1][2] = A[2][1] = S[0][1] + S[1][0];
    A[1][3] = A[3][1] = S[2][0] + S[0][2];
    A[2][3] = A[3][2] = S[1][2] + S[2][1];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kSweeps; ++sweep) {
        if (A[0][1] == 0.0 && A[0][2] == 0.0 && A[0][3] == 0.0 && A[1][2] == 0.0 && A[1][3] == 0.0 && A[2][3] == 0.0) break;
        rotate<0, 1>(A, V);
        rotate<0, 2>(A, V);
        rotate<0, 3>(A, V);
        rotate<1, 2>(A, V);
        rotate<1, 3>(A, V);
        rotate<2, 3>(A, V);
    }
    // the first of the largest diagonal entries
    double best = A[0][0], w = V[0][0], x = V[1][0], y = V[2][0], z = V[3][0];
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (A[k][k] > best) {
            best = A[k][k];
            w = V[0][k];
            x = V[1][k];
            y = V[2][k];
            z = V[3][k];
        }
    const double len = sqrt(((w * w + x * x) + y * y) + z * z);
    w = w / len;
    x = x / len;
    y = y / len;
    z = z / len;
    const double ww = w * w, xx = x * x, yy = y * y, zz = z * z;
    R[0] = ((ww + xx) - yy) - zz;
    R[1] = 2.0 * (x * y - w * z);
    R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);
    R[4] = ((ww - xx) + yy) - zz;
    R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);
    R[7] = 2.0 * (y * z + w * x);
    R[8] = ((ww - xx) - yy) + zz;
}

}  // namespace
