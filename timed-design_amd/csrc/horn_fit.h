// The one least-squares superposition of th_superpose (superpose.hip), th_tmscore (tmscore.hip) and th_cealign (cealign.hip):
// Fit is its state, moved = R (mob - cm) + cr; distance() and store() are the only places that expression and its [R | t] form are
// written; add_position() and add_covariance() are the two accumulation steps on a lane's own partial sums; wave_fit() runs them
// lane-strided over one 64-lane wavefront with device_math.h's wave_sum between them (k_ce_best runs them serially, in path order,
// itself); horn_rotation() is one cyclic Jacobi and Horn's quaternion route from the 3 x 3 cross-covariance to the proper
// rotation.  Every lane computes the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include "device_math.h"

// every float64 product and sum below is rounded separately, as the NumPy restatement's are
#pragma clang fp contract(off)

namespace {

constexpr int kWave = 64;
constexpr int kSweeps = 10;                       // Jacobi sweeps at most (a 4 x 4 matrix is diagonal to the last bit after 5 or 6)

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

// a superposition: moved = R (mob - cm) + cr, R row-major; the identity until something has been fitted
struct Fit {
    double cm[3] = {0.0, 0.0, 0.0}, cr[3] = {0.0, 0.0, 0.0};
    double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
};

// the distance of one position pair (three doubles each) under f
__device__ inline double distance(const Fit& f, const double* ref, const double* mob) {
    const double ax = mob[0] - f.cm[0], ay = mob[1] - f.cm[1], az = mob[2] - f.cm[2];
    const double dx = (((f.R[0] * ax + f.R[1] * ay) + f.R[2] * az) + f.cr[0]) - ref[0];
    const double dy = (((f.R[3] * ax + f.R[4] * ay) + f.R[5] * az) + f.cr[1]) - ref[1];
    const double dz = (((f.R[6] * ax + f.R[7] * ay) + f.R[8] * az) + f.cr[2]) - ref[2];
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

// f as the 12 doubles [R | t] of moved = R mob + t, t = cr - R cm
__device__ inline void store(const Fit& f, double* t) {
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        t[4 * x] = f.R[3 * x];
        t[4 * x + 1] = f.R[3 * x + 1];
        t[4 * x + 2] = f.R[3 * x + 2];
        t[4 * x + 3] = f.cr[x] - ((f.R[3 * x] * f.cm[0] + f.R[3 * x + 1] * f.cm[1]) + f.R[3 * x + 2] * f.cm[2]);
    }
}

// the two passes of a fit over one position pair: the sums behind the centroids, then the cross-covariance of the centred pair
__device__ inline void add_position(const double* ref, const double* mob, double (&sr)[3], double (&sm)[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        sm[a] += mob[a];
        sr[a] += ref[a];
    }
}

__device__ inline void add_covariance(const Fit& f, const double* ref, const double* mob, double (&S)[3][3]) {
    double a[3], b[3];
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        a[x] = mob[x] - f.cm[x];
        b[x] = ref[x] - f.cr[x];
    }
#pragma unroll
    for (int x = 0; x < 3; ++x)
#pragma unroll
        for (int y = 0; y < 3; ++y) S[x][y] += a[x] * b[y];
}

// The fit of one wavefront over `count` selected positions of ref / mob.  each(visit) calls visit(i) for the selected positions i
// that this lane owns, in increasing order: the order of a lane's own additions; the lanes then meet in wave_sum's butterfly.
template <class Each>
__device__ inline void wave_fit(const double* ref, const double* mob, Each each, double count, Fit& f) {
    double sr[3] = {0.0, 0.0, 0.0}, sm[3] = {0.0, 0.0, 0.0};
    each([&](auto i) { add_position(ref + 3 * i, mob + 3 * i, sr, sm); });
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        f.cm[a] = wave_sum(sm[a]) / count;
        f.cr[a] = wave_sum(sr[a]) / count;
    }
    double S[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};          // two-pass: of the centred coordinates
    each([&](auto i) { add_covariance(f, ref + 3 * i, mob + 3 * i, S); });
#pragma unroll
    for (int x = 0; x < 3; ++x)
#pragma unroll
        for (int y = 0; y < 3; ++y) S[x][y] = wave_sum(S[x][y]);
    horn_rotation(S, f.R);
}

}  // namespace
