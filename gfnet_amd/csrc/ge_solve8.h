// ge_solve8.h -- the 8x8 Gaussian elimination shared by the homography solve (homography.hip: RANSAC hypotheses and the
// Levenberg-Marquardt steps) and the four-point perspective solves of the pair synthesis (pair_synth.hip).
#pragma once
#include "common.h"

namespace gfn {

// value of `v` in lane `srclane`.  UNIFORM: srclane is wave-uniform -> two v_readlane_b32 (a few
// cycles); otherwise a general shuffle (ds_bpermute, LDS crossbar latency).
template <bool UNIFORM>
__device__ __forceinline__ double lane_get(double v, int srclane) {
    if (UNIFORM) {
        const int lo = __builtin_amdgcn_readlane(__double2loint(v), srclane);
        const int hi = __builtin_amdgcn_readlane(__double2hiint(v), srclane);
        return __hiloint2double(hi, lo);
    }
    return __shfl(v, srclane);
}

// Gaussian elimination with partial pivoting of an 8x8 system, one augmented row (9 doubles) per
// lane: lanes base..base+7 of the wave hold rows 0..7.  Same operation order as solve_aug() in the
// oracle.  Returns the solution component of this lane's row; ok is group-uniform.
// UNIFORM = the wave holds a single system (base is wave-uniform).
template <bool UNIFORM>
__device__ double ge_solve8(double (&M)[9], int row, int base, bool &ok) {
    ok = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        int piv = c;
        double best = fabs(lane_get<UNIFORM>(M[c], base + c));
#pragma unroll
        for (int r = c + 1; r < 8; ++r) {
            const double v = fabs(lane_get<UNIFORM>(M[c], base + r));
            if (v > best) { best = v; piv = r; }
        }
        if (!(best > 1e-300)) ok = false;
        if (UNIFORM) piv = __builtin_amdgcn_readfirstlane(piv);
        // swap rows c and piv (every lane takes part in the exchange)
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const double from_piv = lane_get<UNIFORM>(M[k], base + piv), from_c = lane_get<UNIFORM>(M[k], base + c);
            M[k] = (row == c) ? from_piv : ((row == piv) ? from_c : M[k]);
        }
        const double inv = 1.0 / lane_get<UNIFORM>(M[c], base + c);
        const double f = M[c] * inv;
#pragma unroll
        for (int k = c; k < 9; ++k) {
            const double prow = lane_get<UNIFORM>(M[k], base + c);
            if (row > c) M[k] = M[k] - f * prow;
        }
    }
    double s = M[8];
    double x = 0.0;
#pragma unroll
    for (int k = 7; k >= 0; --k) {
        // lane k finalises x_k = s / M[k][k]; every row above it (row < k) eliminates it
        const double xk = lane_get<UNIFORM>(s / M[k], base + k);
        if (row == k) x = xk;
        if (row < k) s = s - M[k] * xk;
    }
    return x;
}

}  // namespace gfn
