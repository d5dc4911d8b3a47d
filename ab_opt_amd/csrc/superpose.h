// Best-fit superposition of two paired point lists by ONE lane: Horn's closed form (1987) with a cyclic Jacobi solve of the 4x4 key
// matrix, in double.  superpose_pair is the pair function of abopt_superposed_rmsd (superpose.hip) and of abopt_cluster_shapes_grouped (cluster.hip); dockq.hip
// takes jacobi4_max_eigvec from here for its block-wide fit_and_rmsd.  A lane walks its points serially in index order and exchanges nothing with other lanes,
// so the result is a pure function of the two lists: it does not depend on the lane, wave, workgroup or entry point that evaluated it.
#pragma once
#include <math.h>

namespace abopt {

// Largest-eigenvalue eigenvector of the symmetric 4x4 matrix N (cyclic Jacobi, double): Horn's unit quaternion of the best rotation.
__device__ void jacobi4_max_eigvec(double N[4][4], double q[4]) {
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    for (int sweep = 0; sweep < 16; ++sweep) {
        double off = 0;
        for (int i = 0; i < 4; ++i) for (int j = i + 1; j < 4; ++j) off += N[i][j] * N[i][j];
        if (off < 1e-30) break;
        for (int p = 0; p < 3; ++p)
            for (int r = p + 1; r < 4; ++r) {
                if (fabs(N[p][r]) < 1e-300) continue;
                const double theta = (N[r][r] - N[p][p]) / (2.0 * N[p][r]);
                const double tt = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
                for (int k = 0; k < 4; ++k) { const double a = N[k][p], b = N[k][r]; N[k][p] = c * a - s * b; N[k][r] = s * a + c * b; }
                for (int k = 0; k < 4; ++k) { const double a = N[p][k], b = N[r][k]; N[p][k] = c * a - s * b; N[r][k] = s * a + c * b; }
                for (int k = 0; k < 4; ++k) { const double a = V[k][p], b = V[k][r]; V[k][p] = c * a - s * b; V[k][r] = s * a + c * b; }
            }
    }
    // the column of the largest diagonal entry (the first of equals), picked by selects: an index computed at run time would put V into scratch memory
    double top = N[0][0];
    for (int k = 0; k < 4; ++k) q[k] = V[k][0];
    for (int i = 1; i < 4; ++i)
        if (N[i][i] > top) {
            top = N[i][i];
            for (int k = 0; k < 4; ++k) q[k] = V[k][i];
        }
}

// x is the mobile list, y the target.  fx(k, p) / fy(k, p) put the k-th of the nf paired FIT points into double p[3]; sx / sy do so for the ns paired SCORE
// points.  The caller guarantees nf >= 1 (the rotation is determined from nf >= 3 non-collinear points on).
//   centroids   cx, cy = the means of the fit points, summed in double in index order
//   covariance  S[a][b] = sum (x_a - cx_a)(y_b - cy_b) over the fit pairs
//   rotation    the unit quaternion = the largest-eigenvalue eigenvector of Horn's key matrix of S -> R (row-major), a proper rotation, never a reflection
//   residuals   ss = sum |R (x - cx) - (y - cy)|^2 over the score pairs, with the rotation applied (as fit_and_rmsd of dockq.hip does: the eigenvalue identity
//               Gx + Gy - 2 lambda cannot serve a score set other than the fit set, and loses half its digits where the RMSD is near 0)
//   t = cy - R cx, so that y ~ R x + t
// -> ss.  With COLLINEAR fit points (or fewer than three) the two largest eigenvalues coincide and the rotation is that of SOME optimal fit: whatever turn about
// the points' line the Jacobi sweeps leave.  ss over the fit points themselves is the same for every optimal rotation; ss over other points is not.
// Every product that feeds a sum is an explicit fma and the block is compiled with contraction off, so each copy of this function rounds alike; the Jacobi's
// trip counts are constants (16 sweeps at most), so it ends whatever the data, NaN included (a NaN in either list gives ss = NaN).
template <class FX, class FY, class SX, class SY>
__device__ __forceinline__ double superpose_pair(int nf, int ns, FX fx, FY fy, SX sx, SY sy, double R[9], double t[3]) {
#pragma clang fp contract(off)
    double cx[3] = {0, 0, 0}, cy[3] = {0, 0, 0}, p[3], o[3];
    for (int k = 0; k < nf; ++k) {
        fx(k, p); fy(k, o);
#pragma unroll
        for (int a = 0; a < 3; ++a) { cx[a] += p[a]; cy[a] += o[a]; }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) { cx[a] /= (double)nf; cy[a] /= (double)nf; }
    double S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < nf; ++k) {
        fx(k, p); fy(k, o);
#pragma unroll
        for (int a = 0; a < 3; ++a) { p[a] -= cx[a]; o[a] -= cy[a]; }
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) S[a * 3 + b] = fma(p[a], o[b], S[a * 3 + b]);
    }
    const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
    double N[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                      {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                      {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                      {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
    double q[4];
    jacobi4_max_eigvec(N, q);
    const double a = q[0], b = q[1], c = q[2], d = q[3];
    R[0] = a * a + b * b - c * c - d * d; R[1] = 2 * (b * c - a * d); R[2] = 2 * (b * d + a * c);
    R[3] = 2 * (b * c + a * d); R[4] = a * a - b * b + c * c - d * d; R[5] = 2 * (c * d - a * b);
    R[6] = 2 * (b * d - a * c); R[7] = 2 * (c * d + a * b); R[8] = a * a - b * b - c * c + d * d;
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = cy[k] - fma(R[k * 3 + 2], cx[2], fma(R[k * 3 + 1], cx[1], R[k * 3] * cx[0]));
    double ss = 0;
    for (int k = 0; k < ns; ++k) {
        sx(k, p); sy(k, o);
#pragma unroll
        for (int j = 0; j < 3; ++j) { p[j] -= cx[j]; o[j] -= cy[j]; }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double e = fma(R[j * 3 + 2], p[2], fma(R[j * 3 + 1], p[1], R[j * 3] * p[0])) - o[j];
            ss = fma(e, e, ss);
        }
    }
    return ss;
}

// what both entry points report of a pair: (float) sqrt(ss / n)
__device__ __forceinline__ float superposed_rmsd_of(double ss, int n) { return (float)sqrt(ss / (double)n); }

}  // namespace abopt
