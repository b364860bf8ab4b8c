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
#include <algorithm>
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

// ---- the joint threshold ahead of a LIBRARY's prefilter (pfmscan_library_hits_sum_*) --------------------------------
// k_library's phase A needs a finite letters threshold for its credit tables; with a joint threshold T_k one follows
// from an upper bound on the structure score.  Let S be the profile's row bound (pfmscan_profile_row_bound_*: every row
// a scorable window touches has finite entries >= 0 whose fp64 sum, c ascending, is <= S) and P the motif's PSSM with
// no +inf cell.
//   * rows.  The REAL sum of a row's entries is sigma <= s (1 + u)^6 with s its fp64 sum and u = 2^-53 (six rounded
//     additions of non-negative terms); SUM_ROW_UP = 1 + 2^-50 > (1 + u)^6 gives sigma <= S_up = up(S SUM_ROW_UP).
//   * one row-dot.  Row j of P with a NaN or -inf cell: the product with that cell is NaN (NaN cell, or entry 0 times
//     -inf) or -inf, and a sum holding one of them is NaN or -inf, never +inf: nan_to_num gives 0 or -DBL_MAX, both
//     <= 0.  All cells finite: the real dot is sum_c r_c P_jc <= sigma max(0, max_c P_jc).  With hi_j = max(0, max of the
//     cells of row j that are neither NaN nor -inf) every row-dot is, in real arithmetic, <= S_up hi_j.
//   * the window.  U = up(S_up up(sum_j hi_j)) bounds the real score; every operation of the host's evaluation is
//     rounded UP (next_up after each), so U is at least the real bound.  The score the kernel decides on is a computed
//     one, fast (F) or re-scored (R): each is a sum of the same <= 7 m products through at most 7 + m roundings and lies
//     within gamma(8 m) A of the real value, A = sum |r_jc P_jc| <= S_up sum_j max_c |P_jc| (finite cells).
//     err = up(16 m u S_up sum_j max_c |P_jc|) > gamma(8 m) A covers it for ANY S (struct_band only does for entries up
//     to STRUCT_ROW_MAX), and no partial sum overflows to +inf while U + err is finite (the positive part of every partial
//     sum is <= U; an overflow towards -inf only lowers the score).  So  st <= U + max(struct_band, err) =: U + B  for the
//     structure score that enters the decision.
//   * the printed sum is fl(z + st), z = float64(round3(f)) <= f + 0.0005 + 3.01 u32 |f| (above; u32 = 2^-24) for
//     |f| <= ROUND3_SAFE.  f is the float32 of a sequential fp64 sum of m letters: |f| <= Fk (1 + m u)(1 + u32) with
//     Fk = sum_j max_c |L_jc| (finite cells; a window over a -inf cell scores -inf and is no hit), so
//     3.01 u32 |f| <= FT = up(ROUND3_C u32 Fk (1 + 2^-20)).
//     With  e = down(down(down(down(T - U) - B) - 0.0005 (1 + 2^-50)) - FT)  (every subtraction rounded DOWN) a window
//     with f <= e has, in real arithmetic,  z + st <= e + 0.0005 + FT + U + B <= T,  and rounding to fp64 is monotone and T
//     is an fp64 number: fl(z + st) <= T, the window is no hit.  So every hit has (double) f > e as well as > thr_seq:
//         thr_eff = max(thr_seq, e)
//     is a threshold phase A may build its credits for -- a superset filter: the credits never drop a window with
//     (double) f > thr (pfmscan_library_api.hip), and phase B decides with the real thr_seq, thr_struct and T.
//   * no tightening (thr_eff = thr_seq) for a motif with a +inf PSSM cell (no bound), a +inf / NaN letter cell (the
//     prefilter is off for it anyway), Fk > ROUND3_SAFE (the round3 bound does not hold), S = +inf or NaN (no promise
//     about the rows), T = -inf, or whenever e comes out NaN.
constexpr double SUM_ROW_UP = 1.0 + 0x1p-50;
inline double next_up(double x) { return std::nextafter(x, INFINITY); }
inline double next_down(double x) { return std::nextafter(x, -INFINITY); }

// host: the pieces of the bound for one motif: letters [m][8] (columns 0..3 count), pssm [m][7]
struct SumBound {
    double U = 0.0, B = 0.0, FT = 0.0, Fk = 0.0;
    bool ok = false;                           // false: one of the switch-off conditions holds
};
inline SumBound sum_bound(const double *letters, const double *pssm, int m, double row_sum_max)
{
    SumBound b;
    if (!(row_sum_max >= 0.0) || !(row_sum_max < INFINITY)) return b;
    double hi_sum = 0.0, abs_sum = 0.0, fk = 0.0;
    for (int j = 0; j < m; ++j) {
        double hi = 0.0, mx = 0.0, lmx = 0.0;
        for (int c = 0; c < 7; ++c) {
            const double p = pssm[j * 7 + c];
            if (p == INFINITY) return b;
            if (std::isnan(p) || p == -INFINITY) continue;
            hi = std::max(hi, p);
            mx = std::max(mx, std::fabs(p));
        }
        for (int c = 0; c < 4; ++c) {
            const double l = letters[j * 8 + c];
            if (std::isnan(l) || l == INFINITY) return b;
            if (l > -INFINITY) lmx = std::max(lmx, std::fabs(l));
        }
        hi_sum = next_up(hi_sum + hi);
        abs_sum = next_up(abs_sum + mx);
        fk = next_up(fk + lmx);
    }
    if (!(fk <= ROUND3_SAFE)) return b;
    const double s_up = next_up(row_sum_max * SUM_ROW_UP);
    b.U = next_up(s_up * hi_sum);
    const double err = next_up(next_up(16.0 * (double)m * 0x1p-53 * s_up) * abs_sum);
    b.B = std::max(struct_band(pssm, m), err);
    b.Fk = fk;
    b.FT = next_up(next_up(ROUND3_C * 0x1p-24 * (1.0 + 0x1p-20)) * fk);
    b.ok = true;
    return b;
}
// host: the letters threshold phase A of a library may use for one motif under the joint threshold thr_sum
inline double sum_thr_eff(const double *letters, const double *pssm, int m, double thr_seq, double thr_sum, double row_sum_max)
{
    if (!(thr_sum > -INFINITY)) return thr_seq;
    if (thr_sum == INFINITY) return INFINITY;              // nothing exceeds +inf
    const SumBound b = sum_bound(letters, pssm, m, row_sum_max);
    if (!b.ok) return thr_seq;
    double e = next_down(thr_sum - b.U);
    e = next_down(e - b.B);
    e = next_down(e - 0.0005 * (1.0 + 0x1p-50));
    e = next_down(e - b.FT);
    if (std::isnan(e)) return thr_seq;
    return std::max(thr_seq, e);
}

// np.round(float32, 3), bit for bit: multiply, rint, divide, each rounded to float32 (no contraction, IEEE division).  ONE
// function for both sides: the device spells the multiply and the divide with the round-to-nearest intrinsics, the host's plain
// operators are IEEE float32 already; rintf on either side (round to nearest even, the mode both run in).
__host__ __device__ __forceinline__ float round3(float x)
{
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
    const float y = __fmul_rn(x, 1000.0f);
    const float r = rintf(y);
    return __fdiv_rn(r, 1000.0f);
#else
    const float y = x * 1000.0f;
    const float r = rintf(y);
    return r / 1000.0f;
#endif
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

// ---- the joint threshold of the two-FASTA mode (pfmscan_hits_pair_sum_*) ---------------------------------------------
// Both scores are letter sums here and BOTH printed columns are rounded (scan_pair.rows; rnascan.py:273, :416-434):
//     printed(p) = fl( (double) round3(f) + round3d(st) ),   f = float32 of the sequence sum, st = the fp64 structure sum.
// There is no near band and no re-score: st already is the reference-order value.
//
// round3d(x) = Python's round(x, 3) of a double = the double nearest to the 3-digit decimal nearest to the EXACT binary
// value, ties to even (float.__round__ goes through dtoa / strtod; pfmscan_round_decimals is the host's form of it).
// Without strings, for |fl(1000 x)| < 2^52:  y = fl(1000 x) and e = fma(x, 1000, -y) give the product exactly, y + e
// with |e| <= ulp(y) / 2;  r = rint(y);  t = y - r is exact and a multiple of ulp(y) <= 1/2.  When |t| < 1/2, y is at least
// ulp(y) away from the nearest half-integer and |e| <= ulp(y) / 2 cannot carry the product to or across it: r is the
// product's nearest integer too.  When |t| = 1/2, y IS the half-integer and the sign of e alone says on which side the
// product lies: t = +1/2 with e > 0 -> r + 1, t = -1/2 with e < 0 -> r - 1, e = 0 -> an exact tie, and rint chose the even
// one.  r / 1000 is then ONE correctly rounded division of two exact integers.  From 2^52 on (and for inf / NaN) x comes
// back unchanged, as from pfmscan_round_decimals.
__host__ __device__ inline double round3d(double x)
{
#pragma clang fp contract(off)
    const double y = x * 1000.0;
    if (!(fabs(y) < 0x1p52)) return x;
    const double e = fma(x, 1000.0, -y);
    double r = rint(y);
    const double t = y - r;
    if (t == 0.5 && e > 0.0) r += 1.0;
    else if (t == -0.5 && e < 0.0) r -= 1.0;
    return r / 1000.0;
}

// Cheap superset test ahead of the two roundings and the division: a window goes on only if
//     fl( fl((double) f + st) + mg ) > thr_sum,   mg = margin0 + ROUND3_C u32 |f| + 2^-50 |st|      (u32 = 2^-24, u = 2^-53).
// Why no window whose printed sum passes fails it.  fl(z + s3) > T with T a double implies z + s3 > T in real numbers
// (rounding is monotone).  z = (double) round3(f) <= f + 0.0005 + 3.01 u32 |f| for |f| <= ROUND3_SAFE (head of this file);
// s3 = fl(r / 1000) with |r / 1000 - st| <= 0.0005, so s3 <= st + 0.0005 + u (|st| + 0.0005); a = fl(f + st) >= f + st -
// u (|f| + |st|).  Together  a + M > T  with  M = 0.001 + 3.01 u32 |f| + u |f| + 2 u |st| + 2^-63.  The computed mg (two FMAs,
// each within 2^-53 relative) exceeds M by at least 0.001 (2^-50 - 2^-52) - 2^-63 + 2^-50 |T| + 0.98 u32 |f| + 2^-51 |st|
// (margin0 = up(up(0.001 (1 + 2^-50)) + up(2^-50 |T|)), pair_sum_margin0), so a + mg > T + 2^-50 |T| >= T + 2 ulp(T) in
// real numbers and its rounding is still > T.  Beyond ROUND3_SAFE (and for +inf) the test is skipped, not trusted.
inline double pair_sum_margin0(double thr_sum)
{
    if (!std::isfinite(thr_sum)) return 0.0;
    return next_up(next_up(0.001 * (1.0 + 0x1p-50)) + next_up(0x1p-50 * std::fabs(thr_sum)));
}
// host: an upper bound Mmax on (printed-sum margin + the roundings of the test's two additions) for EVERY window of one pair, so
// that a hit has (double) f + st > thr_sum - Mmax in real numbers: Mmax = 0.0010001 + 4.01 * 2^-24 F1 + 2^-48 (F1 + F2 + |thr_sum|)
// with F1 / F2 = sum_j max_c |cell| of the sequence / structure table over finite cells (|f| <= F1 (1 + 2^-23), |st| <= F2 (1 + m 2^-53));
// every operation rounded up.  The joint credits of k_pair_cred_sum and thr_eff of a two-FASTA library both start from it.
inline double pair_joint_margin(double F1, double F2, double thr_sum)
{
    double M = next_up(0.0010001 + next_up(4.01 * 0x1p-24 * F1));
    return next_up(M + next_up(0x1p-48 * next_up(next_up(F1 + F2) + std::fabs(thr_sum))));
}
// host: the letters threshold phase A of a TWO-FASTA library may use for one pair under the joint threshold thr_sum
// (pfmscan_library_hits_letters_sum_*).  The structure score is a letter sum here: st <= U2 = the sequential fp64 sum, j ascending,
// of the row maxima of table2 over finite cells -- the very sum the kernel takes for the window that holds those letters, so U2 is
// ATTAINED (rounding is monotone: a window with smaller cells sums to no more), not merely a bound.  A hit has
// (double) f + st > thr_sum - Mmax (pair_joint_margin), hence (double) f > e = down(down(thr_sum - Mmax) - U2), and
//     thr_eff = max(thr_seq, e)
// is a superset threshold for the credits; phase B decides with the caller's thr_seq, thr_struct and thr_sum.  No tightening
// (thr_eff = thr_seq) with a +inf cell in table2 (no bound), a +inf / NaN cell in the letter columns of table1 (the prefilter is
// off for it anyway), letters beyond ROUND3_SAFE, thr_sum = -inf, or when e comes out NaN.  A row of table2 without a finite cell
// makes every window -inf / NaN: it adds nothing to U2.
inline double pair_thr_eff(const double *table1, const double *table2, int m, double thr_seq, double thr_sum)
{
    if (!(thr_sum > -INFINITY)) return thr_seq;
    if (thr_sum == INFINITY) return INFINITY;
    double F1 = 0.0, F2 = 0.0, U2 = 0.0;
    for (int j = 0; j < m; ++j) {
        double mx1 = 0.0, mx2 = 0.0, hi = -INFINITY;
        for (int c = 0; c < 4; ++c) {
            const double l = table1[j * 8 + c];
            if (std::isnan(l) || l == INFINITY) return thr_seq;
            if (l > -INFINITY) mx1 = std::max(mx1, std::fabs(l));
        }
        for (int c = 0; c < 8; ++c) {
            const double v = table2[j * 8 + c];
            if (v == INFINITY) return thr_seq;
            if (std::isfinite(v)) {
                mx2 = std::max(mx2, std::fabs(v));
                hi = std::max(hi, v);
            }
        }
        F1 = next_up(F1 + mx1);
        F2 = next_up(F2 + mx2);
        if (hi > -INFINITY) U2 = U2 + hi;              // the kernel's own order and rounding
    }
    if (!(F1 <= ROUND3_SAFE)) return thr_seq;
    const double e = next_down(next_down(thr_sum - pair_joint_margin(F1, F2, thr_sum)) - U2);
    if (std::isnan(e)) return thr_seq;
    return std::max(thr_seq, e);
}
__host__ __device__ inline bool pair_sum_maybe(float f, double st, double thr_sum, double margin0)
{
#pragma clang fp contract(off)
    const double x = (double)f;
    const double mg = fma(fabs(st), 0x1p-50, fma(fabs(x), ROUND3_C * 0x1p-24, margin0));
    return !(fabs(x) <= ROUND3_SAFE) || ((x + st) + mg > thr_sum);
}
// The third predicate for a window that already passed f > thr_seq AND st > thr_struct (so neither is NaN or -inf).
__host__ __device__ inline bool pair_sum_passes(float f, double st, double thr_sum, double margin0)
{
#pragma clang fp contract(off)
    if (!pair_sum_maybe(f, st, thr_sum, margin0)) return false;
    return (double)round3(f) + round3d(st) > thr_sum;
}

}  // namespace pfmscan
