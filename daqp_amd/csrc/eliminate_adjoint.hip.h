// eliminate_adjoint.hip.h -- the adjoint of an eliminated batch: reduce the right-hand side (k_adjoint_reduce), run the adjoint of the
// reduced batch (backward.hip.h / nullspace.hip.h, unchanged), expand (k_adjoint_expand).  Additive: nothing here runs inside a
// setup, a solve or the adjoint of a batch that was not eliminated.
//
// Per problem, in the notation of eliminate.hip.h (E = C_eq_rows with unit-row QR E' = Q [R; 0], Q = [Q1 Z], row norms s; I the kept
// rows; W_I the stored working set of the reduced batch), for g_x = dl/dx and g_lam = dl/dlam the system at the full working set
// W = E u W_I
//
//     [ H     E'   C_WI' ] [ dz    ]   [ g_x     ]
//     [ E     0    0     ] [ dnu_E ] = [ g_lam_E ]
//     [ C_WI  0    0     ] [ dnu_I ]   [ g_lam_WI]
//
// is solved on the two factors that the forward pass kept:
//
//     reduce    y = R^-T (g_lam_E / s),  dz0 = Q [y; 0],  grad_y = (Q'(g_x - H dz0))[neq:],  grad_lam_r = g_lam_I - C_I dz0 (every
//               kept row; the reduced adjoint reads it on W_I).  g_lam == null: dz0 = 0, grad_y = (Q'g_x)[neq:], no grad_lam_r.
//     solve     the adjoint of the reduced batch on (grad_y, grad_lam_r): dz_r, dbupper_r, dblower_r, status_r
//     expand    dz = dz0 + Q [0; dz_r],  dnu_I = dbupper_r + dblower_r (each at its original row, on the side the reduced call chose),
//               R dnu~ = (Q'(g_x - H dz - C_WI' dnu_I))[:neq],  dnu_E = dnu~ / s -> dbupper of the equality rows (the elimination reads
//               e from bupper), dblower = 0 there
//
// -- el_x0 / el_rhs / k_expand with e -> g_lam_E, f -> -g_x, the bounds -> g_lam_I.  An LP batch (d.lp) has H = 0 in every product.
// A problem whose elimination flag is negative gets that flag as its status and zero outputs; every other problem gets status_r, with
// zero outputs where that is non-zero.
//
// Mapping: k_expand's -- one wavefront per problem at every n <= 511, NV = ceil(n / 64) entries per lane, one n-vector of static LDS
// for the H product; the kept factor is read from global memory.  g_lam_I - C_I dz0 is one butterfly dot product per kept row, the
// rows taken one after the other by the wavefront (el_rhs's loop with W = 1, as k_eliminate_update runs it): a row is read once,
// coalesced, and dz0 stays in registers.  All arithmetic is fp64, no contraction.
#pragma once
#include "eliminate.hip.h"

namespace daqp_amd {

struct ElimAdjointArgs {
    const double *grad_x, *grad_lam;               // [N][n], [N][m]: the caller's; either may be null (= 0)
    double *grad_y, *grad_lam_r, *dz0;             // [N][nr], [N][mr], [N][n]: the handle's; the last two unused when grad_lam is null
    double *dz_r, *dbu_r, *dbl_r;                  // [N][nr], [N][mr], [N][mr]: the handle's, written by the reduced adjoint
    int *status_r;                                 // [N]
    double *dz, *dbupper, *dblower;                // [N][n], [N][m], [N][m]: the caller's
    int *status;                                   // [N]
};

template <int NV>
__global__ __launch_bounds__(64) void k_adjoint_reduce(ElimDev d, ElimAdjointArgs a)
{
    __shared__ double xs[64 * NV];
    const int lane = threadIdx.x, q = blockIdx.x, n = d.n, m = d.m, neq = d.neq, nr = d.nr, mr = d.mr, ldn = d.ldn;
    if (q >= d.N || n > 64 * NV) return;
    if (d.flags[q] < 0) {      // no factor, or no equality problem: a zero right-hand side for whatever the reduced batch holds there
        for (int i = lane; i < nr; i += 64) a.grad_y[(size_t)q * nr + i] = 0.0;
        if (a.grad_lam) for (int j = lane; j < mr; j += 64) a.grad_lam_r[(size_t)q * mr + j] = 0.0;
        return;
    }
    const double *V = d.V + (size_t)q * neq * ldn, *beta = d.beta + (size_t)q * neq, *rd = d.rd + (size_t)q * neq, *rn = d.rn + (size_t)q * neq;
    double g[NV];
#pragma unroll
    for (int e = 0; e < NV; ++e) {
        const int i = lane + 64 * e;
        g[e] = (a.grad_x && i < n) ? a.grad_x[(size_t)q * n + i] : 0.0;
    }
    double z0[NV];
    if (a.grad_lam) {
        // dz0 = Q [R^-T (g_lam_E / s); 0]: el_x0 with g_lam where it reads e
        ElimDev dg = d;
        dg.bu = a.grad_lam;
        el_x0<NV>(z0, dg, q, V, beta, rd, rn, lane);
#pragma unroll
        for (int e = 0; e < NV; ++e) {
            const int i = lane + 64 * e;
            if (i < n) { xs[i] = z0[e]; a.dz0[(size_t)q * n + i] = z0[e]; }
        }
        __syncthreads();
        if (!d.lp) {
            double t[NV];
            el_hmul<NV>(t, d.H + (size_t)q * n * n, xs, lane, n);
#pragma unroll
            for (int e = 0; e < NV; ++e) g[e] -= t[e];
        }
    }
    // grad_y = (Q'(g_x - H dz0))[neq:]
    for (int c = 0; c < neq; ++c) el_reflect<NV>(g, V, beta, c, ldn, lane, n);
#pragma unroll
    for (int e = 0; e < NV; ++e) {
        const int i = lane + 64 * e;
        if (i >= neq && i < n) a.grad_y[(size_t)q * nr + (i - neq)] = g[e];
    }
    if (!a.grad_lam) return;
    // grad_lam_r = g_lam_I - C_I dz0
    for (int j = 0; j < mr; ++j) {
        const int r = d.kept[j];
        double crow[NV];
        el_row<NV>(crow, d, q, r, lane);
        const double cz = el_dot<NV>(crow, z0);
        if (lane == 0) a.grad_lam_r[(size_t)q * mr + j] = a.grad_lam[(size_t)q * m + r] - cz;
    }
}

template <int NV>
__global__ __launch_bounds__(64) void k_adjoint_expand(ElimDev d, ElimAdjointArgs a)
{
    __shared__ double xs[64 * NV];
    const int lane = threadIdx.x, q = blockIdx.x, n = d.n, m = d.m, neq = d.neq, nr = d.nr, mr = d.mr, ldn = d.ldn;
    if (q >= d.N || n > 64 * NV) return;
    const int flag = d.flags[q];
    const int st = flag < 0 ? flag : a.status_r[q];
    if (lane == 0) a.status[q] = st;
    if (st != 0) {
        for (int i = lane; i < n; i += 64) a.dz[(size_t)q * n + i] = 0.0;
        for (int r = lane; r < m; r += 64) { a.dbupper[(size_t)q * m + r] = 0.0; a.dblower[(size_t)q * m + r] = 0.0; }
        return;
    }
    const double *V = d.V + (size_t)q * neq * ldn, *beta = d.beta + (size_t)q * neq, *rd = d.rd + (size_t)q * neq, *rn = d.rn + (size_t)q * neq;
    // dz = dz0 + Q [0; dz_r]
    double x[NV];
#pragma unroll
    for (int e = 0; e < NV; ++e) {
        const int i = lane + 64 * e;
        x[e] = (i >= neq && i < n) ? a.dz_r[(size_t)q * nr + (i - neq)] : 0.0;
    }
    for (int c = neq - 1; c >= 0; --c) el_reflect<NV>(x, V, beta, c, ldn, lane, n);
#pragma unroll
    for (int e = 0; e < NV; ++e) {
        const int i = lane + 64 * e;
        if (i < n) {
            if (a.grad_lam) x[e] += a.dz0[(size_t)q * n + i];
            xs[i] = x[e];
            a.dz[(size_t)q * n + i] = x[e];
        }
    }
    __syncthreads();
    for (int j = lane; j < mr; j += 64) {      // every row is written once: the kept ones here, the equality rows at the end
        const size_t k = (size_t)q * m + d.kept[j];
        a.dbupper[k] = a.dbu_r[(size_t)q * mr + j];
        a.dblower[k] = a.dbl_r[(size_t)q * mr + j];
    }
    // g = g_x - H dz - C_WI' dnu_I
    double g[NV];
    if (d.lp) {
#pragma unroll
        for (int e = 0; e < NV; ++e) g[e] = 0.0;
    } else el_hmul<NV>(g, d.H + (size_t)q * n * n, xs, lane, n);
#pragma unroll
    for (int e = 0; e < NV; ++e) {
        const int i = lane + 64 * e;
        g[e] = ((a.grad_x && i < n) ? a.grad_x[(size_t)q * n + i] : 0.0) - g[e];
    }
    const double *Aq = d.A + (size_t)q * (m - d.ms) * n;
    for (int j = 0; j < mr; ++j) {
        const double l = a.dbu_r[(size_t)q * mr + j] + a.dbl_r[(size_t)q * mr + j];      // (wave-uniform)
        if (l == 0.0) continue;
        const int r = d.kept[j];
#pragma unroll
        for (int e = 0; e < NV; ++e) {
            const int i = lane + 64 * e;
            if (i < n) g[e] -= (r < d.ms ? (i == r ? 1.0 : 0.0) : Aq[(size_t)(r - d.ms) * n + i]) * l;
        }
    }
    // R dnu~ = (Q'g)(0:neq), column by column; dnu_E = dnu~ / |row|
    for (int c = 0; c < neq; ++c) el_reflect<NV>(g, V, beta, c, ldn, lane, n);
    for (int c = neq - 1; c >= 0; --c) {
        const double dc = el_bcast<NV>(g, c) / rd[c];
#pragma unroll
        for (int e = 0; e < NV; ++e) {
            const int i = lane + 64 * e;
            if (i == c) g[e] = dc;
            else if (i < c) g[e] -= V[(size_t)c * ldn + i] * dc;
        }
    }
#pragma unroll
    for (int e = 0; e < NV; ++e) {
        const int i = lane + 64 * e;
        if (i < neq) {
            const size_t k = (size_t)q * m + d.eq_rows[i];
            a.dbupper[k] = g[e] / rn[i];
            a.dblower[k] = 0.0;
        }
    }
}

} // namespace daqp_amd
