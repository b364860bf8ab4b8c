// pfmscan_exact.hpp -- the decision `structure score > threshold` (rnascan.py:310) taken the way the reference's own
// arithmetic takes it, for every thresholded structure path (k_profile / k_profile_fixed hits, k_struct_at, k_wide,
// k_library phase B, k_profile_lib).  Not installed.
//
// The reference scores a window as  score += nan_to_num(np.dot(profile[i + j, :], pssm[j, :]))  (rnascan.py:302-307): each
// row-dot is ROUNDED, then added.  np.dot's own order is BLAS-defined; the restatement the parity tests pin (goldens from
// the reference run here) takes it k-ascending with every product and every addition rounded separately.  The kernels do
// not: a row is one multiply and six FMAs, and with an all-finite PSSM the seven FMAs go straight into the window sum --
// same terms, same order, results within ~1e-14 (the contract for scores is 1e-6), but a different LAST bit.  For the
// scores that is all there is to say; for HIT POSITIONS it would mean that a window whose score sits within a rounding
// error of the threshold can fall on either side.  So every hits path decides in two steps:
//   1. fast score F as before;
//   2. only if |F - thr| <= band: the window is scored again in the rounded, k-ascending order (struct_window_rounded)
//      and THAT value is compared and reported.
// band (struct_band, host) bounds |F - rounded| rigorously: both are sums of the same <= 7 m products in which every
// term passes through at most 7 + m roundings, so each differs from the exact sum by at most gamma(8 m) A with
// A = sum |r_jk P_jk| <= max|r| sum |P_jk| over the finite cells; band = 24 m 2^-53 STRUCT_ROW_MAX sum |P_jk| (> 2 gamma(8 m) A).
// Profile entries are probabilities; the bound holds for any |entry| <= STRUCT_ROW_MAX = 1024.  Non-finite rows and cells
// take the same nan_to_num values in both orders (0, +-DBL_MAX) and drop out of the difference.  The band is ~1e-10
// score units at w = 12: the second step runs for one window in ~10^11.
//
// The joint threshold  LogOdds.SeqStruct > thr_sum  (rnascan.py:416-434 adds the two printed columns; pfmscan_hits_sum_*)
// is decided the same way, on the PRINTED sum  S = float64(round3(seq)) + structure score, one rounded fp64 addition:
//   * round3(x) = np.round(float32 x, 3) = rint(x * 1000f) / 1000f, the three steps each rounded to float32 (round3 below).
//     With u = 2^-24, y = fl(1000 x) = 1000 x (1 + d1), r = rint(y) = y + e (|e| <= 1/2; e = 0 from |y| >= 2^23 on) and
//     z = fl(r / 1000) = (r / 1000)(1 + d2):   z - x = x d1 + e / 1000 + d2 (x (1 + d1) + e / 1000),  so
//         |round3(x) - x| <= 0.0005 (1 + u) + |x| u (2 + u)  <=  0.0005 + c u |x|   with c = 3 once |x| >= 0.0005 / (1 - u).
//     Below that r is 0 or +-1: r = 0 gives |z - x| = |x| <= 0.0005 / (1 - u) <= 0.0005 + 2 u |x|; r = +-1 needs
//     |x| >= 0.0005 (1 - u) and gives |z - x| <= 0.001 (1 + u) - 0.0005 (1 - u) = 0.0005 + 0.0015 u <= 0.0005 + 3.01 u |x|.
//     ROUND3_C = 4 leaves u |x| of slack for the fp64 roundings of the test itself.  The bound needs 1000 x to stay
//     finite: |x| <= ROUND3_SAFE; beyond it (and for NaN) the cheap test is skipped, not trusted.
//   * cheap superset test (sum_maybe): fl(fl(x + margin(x)) + F) > thr_sum with the FAST structure score F and
//     margin(x) = sum_band + 0.0005 + ROUND3_C u |x|.  x + margin(x) >= round3(x) + sum_band in exact arithmetic with
//     u |x| (or 0.00025) to spare, rounding is monotone, and |F - rounded| <= struct_band <= sum_band: no window whose
//     printed sum passes -- with F or with the re-scored value -- fails it.  Only its passers pay the float division.
//   * near band of the sum (sum_band, host): the decision can differ between F and the rounded score R only if
//     fl(z + F) and fl(z + R) lie on different sides of thr_sum.  |F - R| <= struct_band and each addition rounds by at
//     most 2^-53 of a value of magnitude <= |thr_sum| + struct_band (+ one ulp), so then
//         |fl(z + F) - thr_sum| <= struct_band (1 + 2^-52) + 2^-52 |thr_sum| (1 + 2^-52);
//     sum_band = struct_band (1 + 2^-40) + 2^-51 |thr_sum| covers it.  Inside the band the window is scored again
//     (struct_window_rounded) and  z + R  is compared and R reported.  A NaN sum is never near; an infinite thr_sum needs
//     no band (-inf: the plain kernels run; +inf: nothing passes).
#pragma once
#include <float.h>
#include <math.h>
#include <cmath>
#include <hip/hip_runtime.h>

namespace pfmscan {

constexpr double STRUCT_ROW_MAX = 1024.0;

// host: half-width of the re-score band of one structure PSSM [m][7] (row-major, any cells)
inline double struct_band(const double *pssm, int m)
{
    double s = 0.0;
    for (int i = 0; i < m * 7; ++i)
        if (std::isfinite(pssm[i])) s += std::fabs(pssm[i]);
    return 24.0 * (double)m * 0x1p-53 * STRUCT_ROW_MAX * s;
}

__device__ __forceinline__ double exact_nan_to_num(double d)       // numpy.nan_to_num defaults (rnascan.py:306)
{
    const double c = fmin(fmax(d, -DBL_MAX), DBL_MAX);
    return (d != d) ? 0.0 : c;
}

// The window's score in the rounded order: rows[j * 7 + k] = profile row j of the window (any address space, float or
// double storage), cell(j, k) = PSSM cell.  Rolled on purpose: this is the one-in-10^11 path.
template <typename ROW_T, typename CellF>
__device__ __forceinline__ double struct_window_rounded(const ROW_T *rows, int m, CellF cell)
{
#pragma clang fp contract(off)
    double score = 0.0;
#pragma unroll 1
    for (int j = 0; j < m; ++j) {
        double d = 0.0;
#pragma unroll 1
        for (int k = 0; k < 7; ++k) {
            const double prod = (double)rows[j * 7 + k] * cell(j, k);       // rounded product ...
            d = d + prod;                                                    // ... rounded sum: no FMA (contract off)
        }
        score = score + exact_nan_to_num(d);
    }
    return score;
}

// true when the fast score cannot decide by itself
__device__ __forceinline__ bool struct_near(double fast, double thr, double band) { return fabs(fast - thr) <= band; }

// ---- the joint threshold on LogOdds.SeqStruct (see the head of this file) ----------------------------------------
constexpr double ROUND3_C = 4.0;               // |round3(x) - x| <= 0.0005 + ROUND3_C 2^-24 |x|  for |x| <= ROUND3_SAFE
constexpr double ROUND3_SAFE = 3.0e35;         // 1000 x stays finite in float32

// host: half-width of the re-score band of the sum for one structure PSSM's struct_band and one thr_sum
inline double sum_band(double struct_band_, double thr_sum)
{
    if (!std::isfinite(thr_sum)) return 0.0;
    return struct_band_ * (1.0 + 0x1p-40) + 0x1p-51 * std::fabs(thr_sum);
}
// host: the constant part of the cheap test's margin (rounded up)
inline double sum_margin0(double sum_band_) { return (0.0005 + sum_band_) * (1.0 + 0x1p-50); }

// np.round(float32, 3), bit for bit: multiply, rint, divide, each rounded to float32 (no contraction, IEEE division)
__device__ __forceinline__ float round3(float x)
{
#pragma clang fp contract(off)
    const float y = __fmul_rn(x, 1000.0f);
    const float r = rintf(y);
    return __fdiv_rn(r, 1000.0f);
}

// false only when the printed sum cannot exceed thr_sum, whichever structure score (fast or re-scored) ends up in it
__device__ __forceinline__ bool sum_maybe(float seq, double st_fast, double thr_sum, double margin0)
{
#pragma clang fp contract(off)
    const double x = (double)seq;
    const double up = x + fma(fabs(x), ROUND3_C * 0x1p-24, margin0);
    return !(fabs(x) <= ROUND3_SAFE) || (up + st_fast > thr_sum);
}

// The whole decision for one window that already passed seq > thr_seq AND struct > thr_struct.  `st` is the structure
// score so far (fast, or already re-scored near thr_struct); rescore() returns struct_window_rounded of the window.
template <typename Rescore>
__device__ __forceinline__ bool sum_passes(float seq, double &st, double thr_sum, double band, double margin0, Rescore rescore)
{
#pragma clang fp contract(off)
    if (!sum_maybe(seq, st, thr_sum, margin0)) return false;
    const double z = (double)round3(seq);
    double s = z + st;
    if (struct_near(s, thr_sum, band)) {
        st = rescore();
        s = z + st;
    }
    return s > thr_sum;
}

}  // namespace pfmscan
