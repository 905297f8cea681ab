// backward.hip.h -- the adjoint of a solved batch: implicit differentiation of the KKT system at the stored working set.
//
// At an optimum with working set W (rows C_W of C = [first ms rows of I; A], unsigned), for an upstream gradient g = dl/dx:
//
//     [ H    C_W' ] [ dz  ]   [ g ]
//     [ C_W  0    ] [ dnu ] = [ 0 ]
//
// evaluated through the LDP's factor H = R'R (R^-1 is what the setup left in BatchDev::Rinv; H is not factored again):
//     w   = R^-T g
//     N_W = C_W R^-1                          rebuilt here, row by row: a simple bound is a row of R^-1, a general row is A_i R^-1
//     (N_W N_W') dnu = N_W w                  Gram matrix of at most n + 1 rows, rows scaled to unit length first (the solver's own
//                                             tolerance zero_tol meets its pivots as it meets the pivots of the solver's LDL'),
//                                             Cholesky in place
//     dz  = R^-1 (w - N_W' dnu)
// The stored LDL' of the solve (L, vecs) and the blocked image Mblk are NOT read: their layout differs per solve kernel family.
//
// Soft rows (SOFT == true: batches created with ns_max > 0).  An active row k with DAQP_SOFT in its sense sits at
// c_k x - b_k = rho_soft q_k lam_k with q_k = c_k H^-1 c_k' = |N_k|^2, so the (2,2) block of the system is -S instead of 0,
// S = diag(rho_soft q_k on the SOFT rows of W, 0 elsewhere):
//     (N_W N_W' + S) dnu = N_W w              on the unnormalised Gram matrix G_kk *= 1 + rho_soft; q_k is G_kk itself (not
//                                             scaling[]: that one has the diag_h and rows < ms special cases), so after the scaling
//                                             to unit rows the diagonal of a SOFT row is 1 + rho_soft
// S depends on H and A through q_k, and the caller needs q_k and u_k = H^-1 c_k' = R^-1 N_k' for those terms of dl/dH, dl/dA and
// dl/drho_soft (include/daqp_amd.h): qsoft[q][id] = q_k, usoft[q][slot] = u_k (unscaled like dz), usoft_id[q][slot] = id, slots in
// working-set order, ns_max = cap - n - 1 of them per problem, unused ones zero / -1.  DAQP_EXIT_SOFT_OPTIMAL is a differentiable
// end state then.  SOFT == false compiles to what the kernel was before soft rows: side[] holds 0 / 1 and nothing below is emitted.
//
// How R^-1 is stored (daqp_batch_read_ldp shows the same): packed upper, row i at roff(i, n); rows < ms are normalised by
// scaling[i] (true row = stored row / scaling[i]) unless H was diagonal (QState::diag_h: rows kept as they are).  The division is
// folded into the vectors that meet those rows (g, the rows of A, the result), so every output is in the caller's unscaled units.
//
// A dual right-hand side (DUAL == true: daqp_batch_backward_dual).  A loss that also depends on the signed multipliers lam_W puts
// g_lamW[k] = grad_lam[WS[k]] into the second block, K [dz; dnu] = [g; g_lamW], and only the Gram system's right-hand side changes:
//     (N_W N_W') dnu = N_W w - g_lamW
// The rows of N_W are rebuilt unscaled (the scaling[] of the rows < ms of R^-1 is folded into them), so g_lamW is already in their
// units and meets the unit-length scaling alone: rhs_k = (N_k w - g_lamW_k) / |N_k|.  grad_x may be null (= 0) there.  With W empty
// grad_lam is not read.  DUAL == false compiles to what the kernel was before.
//
// Both (SOFT && DUAL: daqp_batch_backward_soft_dual).  A loss that also depends on soft_slack = sum_k S_k lam_k^2 (the SOFT rows of W)
// adds its derivative through lam to the second block, with g_s = grad_slack[q] and lam the multipliers of the solve:
//     ghat_lamW[k] = grad_lam[WS[k]] + 2 g_s rho_soft q_k lam_k  on the SOFT rows of W,  grad_lam[WS[k]] elsewhere
//     (N_W N_W' + S) dnu = N_W w - ghat_lamW
// formed where q_k = G_kk is read and kept in y[] (idle until the triangular solves), so the LDS carve-up is that of SOFT alone --
// and that of DUAL alone: gp[] is the buffer every instantiation has.  grad_lam and grad_slack may each be null (= 0).  The part of
// dl/dS_k that does not go through lam (g_s lam_k^2, and the envelope term of fval) is the caller's (include/daqp_amd.h).
//
// Mapping: one workgroup per problem; T = 64 (ONE wavefront, R^-1, the rows and the Gram matrix in LDS) while n <= 64 and all of it
// fits (with ns_max = 0 the working set holds at most 65 rows and it always does) -- and T = 256 beyond, R^-1 streamed from HBM, rows and Gram matrix in LDS where they fit (NL) and
// in a per-WORKGROUP scratch in HBM where they do not (persistent workgroups, problem q, q + grid, ...).  All arithmetic is fp64.
#pragma once
#include "batch_dev.hip.h"

namespace daqp_amd {

struct BackwardArgs {
    const double *grad_x;         // [N][n]
    double *dz, *dbupper, *dblower; // [N][n], [N][m], [N][m]
    int *status;                  // [N]
    double *scratch;              // [grid][scratch_per_wg] (NL == false), or null
    size_t scratch_per_wg;
    double *qsoft, *usoft;        // [N][m], [N][ns_max][n]: SOFT kernels only, each may be null
    int *usoft_id;                // [N][ns_max], may be null
    const double *grad_lam;       // [N][m]: DUAL kernels only (read on W); grad_x may be null there (= 0)
    const double *grad_slack;     // [N]: SOFT && DUAL kernels only, may be null (= 0); grad_lam may be null there as well (= 0)
    const double *lam;            // [N][m]: the signed multipliers of the solve (read on the SOFT rows of W), null iff grad_slack is
};

// LDS of one workgroup in bytes: w, g', rs (n each), rhs, y, sn, dg (cap each), then R^-1 (RL), rows + Gram (NL), ids, side, flag
__host__ __device__ inline size_t backward_lds_bytes(int n, int cap, bool rl, bool nl)
{
    size_t dbl = 3 * (size_t)n + 4 * (size_t)cap;
    if (rl) dbl += (size_t)n * (n + 1) / 2;
    if (nl) dbl += (size_t)cap * (n | 1) + (size_t)tri(cap);
    return dbl * sizeof(double) + (2 * (size_t)cap + 2) * sizeof(int);
}
__host__ __device__ inline size_t backward_scratch_doubles(int n, int cap) { return (size_t)cap * (n | 1) + (size_t)tri(cap); }

template <int T, bool RL, bool NL, bool SOFT, bool DUAL = false>
__global__ __launch_bounds__(T) void k_backward(BatchDev b, BackwardArgs a)
{
    extern __shared__ double lds_bw[];
    const int tid = threadIdx.x, n = b.n, m = b.m, ms = b.ms, cap = b.cap, mA = b.mA;
    const int ldn = n | 1;      // odd row stride: the Gram dot products walk several rows at once
    double *rs = lds_bw, *gp = rs + n, *w = gp + n, *rhs = w + n, *y = rhs + cap, *sn = y + cap, *dg = sn + cap;
    double *p = dg + cap;
    double *Rl = nullptr, *Nr, *G;
    if constexpr (RL) { Rl = p; p += b.rtri; }
    if constexpr (NL) { Nr = p; p += (size_t)cap * ldn; G = p; p += tri(cap); }
    else { Nr = a.scratch + (size_t)blockIdx.x * a.scratch_per_wg; G = Nr + (size_t)cap * ldn; }
    int *ids = reinterpret_cast<int *>(p), *side = ids + cap, *bad = side + cap;

    for (int q = blockIdx.x; q < b.N; q += gridDim.x) {
        const QState *qs = b.qs + q;
        double *dzq = a.dz + (size_t)q * n, *dbu = a.dbupper + (size_t)q * m, *dbl = a.dblower + (size_t)q * m;
        // ---- what the solve left: every read below is block-uniform
        int st = 0, na = qs->n_active;
        {
            const int sflag = qs->setup_flag, uflag = qs->upd_flag, eflag = qs->exitflag;
            if (sflag < 0) st = sflag;
            else if (uflag < 0) st = uflag;
            else if (eflag != DAQP_EXIT_OPTIMAL && !(SOFT && eflag == DAQP_EXIT_SOFT_OPTIMAL)) st = eflag != 0 ? eflag : DAQP_EXIT_UNSUPPORTED;
            else if (qs->n_prox > 0) st = DAQP_EXIT_UNSUPPORTED;
            else if (qs->sing_ind == DAQP_UNCONSTRAINED_OPTIMAL) na = 0;      // the shortcut: W is empty, dz = H^-1 g
            if (st == 0 && (na < 0 || na > cap)) st = DAQP_BACKWARD_SINGULAR;
        }
        for (int r = tid; r < m; r += T) { dbu[r] = 0.0; dbl[r] = 0.0; }
        const int ns = cap - n - 1;      // ns_max of the batch
        if constexpr (SOFT) {
            if (a.qsoft) for (int r = tid; r < m; r += T) a.qsoft[(size_t)q * m + r] = 0.0;
            if (a.usoft) for (int e = tid; e < ns * n; e += T) a.usoft[(size_t)q * ns * n + e] = 0.0;
            if (a.usoft_id) for (int s = tid; s < ns; s += T) a.usoft_id[(size_t)q * ns + s] = -1;
        }
        if (st == 0) {
            const size_t qF = qf(b, q);
            const double *Rg = b.Rinv + qF * b.rtri, *sc = b.scaling + qF * m;
            const double *Aq = b.A + (b.shared ? qF : (size_t)q) * mA * n;
            const double *R = Rg;
            if constexpr (RL) { for (int e = tid; e < b.rtri; e += T) Rl[e] = Rg[e]; R = Rl; }
            const int diag = qs->diag_h;
            const double *g = (DUAL && !a.grad_x) ? nullptr : a.grad_x + (size_t)q * n;
            if (tid == 0) *bad = 0;
            for (int i = tid; i < n; i += T) {
                const double s = (i < ms && !diag) ? 1.0 / sc[i] : 1.0;
                rs[i] = s;
                if constexpr (DUAL) gp[i] = g ? g[i] * s : 0.0;
                else gp[i] = g[i] * s;
            }
            __syncthreads();
            for (int k = tid; k < na; k += T) {
                const int id = b.WS[(size_t)q * cap + k];
                if (id < 0 || id >= m) { ids[k] = 0; side[k] = 0; *bad = 1; }
                else {
                    const int sg = b.sense[(size_t)q * m + id];
                    ids[k] = id;
                    side[k] = (sg & DAQP_LOWER) ? 1 : 0;
                    if constexpr (SOFT) side[k] |= (sg & DAQP_SOFT) ? 2 : 0;      // bit 1: the row carries rho_soft q_k in S
                }
            }
            // ---- w = R^-T g
            for (int j = tid; j < n; j += T) {
                double s = 0;
                for (int i = 0; i <= j; ++i) s += R[roff(i, n) + j] * gp[i];
                w[j] = s;
            }
            __syncthreads();
            if (*bad) st = DAQP_BACKWARD_SINGULAR;
            // ---- rows of N_W = C_W R^-1 (unscaled)
            if (st == 0 && na > 0) {
                for (int e = tid; e < na * n; e += T) {
                    const int k = e / n, j = e - k * n, id = ids[k];
                    double s = 0;
                    if (id < ms) { if (j >= id) s = rs[id] * R[roff(id, n) + j]; }
                    else {
                        const double *row = Aq + (size_t)(id - ms) * n;
                        for (int i = 0; i <= j; ++i) s += (row[i] * rs[i]) * R[roff(i, n) + j];
                    }
                    Nr[(size_t)k * ldn + j] = s;
                }
                __syncthreads();
                // ---- Gram matrix (packed lower) and right-hand side
                for (int e = tid; e < na * na; e += T) {
                    const int k = e / na, l = e - k * na;
                    if (l > k) continue;
                    const double *x1 = Nr + (size_t)k * ldn, *x2 = Nr + (size_t)l * ldn;
                    double s = 0;
                    for (int j = 0; j < n; ++j) s += x1[j] * x2[j];
                    G[tri(k) + l] = s;
                }
                for (int k = tid; k < na; k += T) {
                    const double *x1 = Nr + (size_t)k * ldn;
                    double s = 0;
                    for (int j = 0; j < n; ++j) s += x1[j] * w[j];
                    rhs[k] = s;
                }
                __syncthreads();
                // rows to unit length: G <- S G S, rhs <- S rhs (dnu = S * the solution)
                for (int k = tid; k < na; k += T) {
                    const double d = G[tri(k) + k];
                    if (!(d > 0.0)) { sn[k] = 0.0; *bad = 1; } else sn[k] = 1.0 / sqrt(d);
                    if constexpr (SOFT) { if ((side[k] & 2) && a.qsoft) a.qsoft[(size_t)q * m + ids[k]] = d; }      // q_k = |N_k|^2
                    if constexpr (SOFT && DUAL) {      // ghat_lamW (in y, free until the solve): q_k is in hand here
                        double gh = a.grad_lam ? a.grad_lam[(size_t)q * m + ids[k]] : 0.0;
                        if ((side[k] & 2) && a.grad_slack) gh += 2.0 * a.grad_slack[q] * b.st.rho_soft * d * a.lam[(size_t)q * m + ids[k]];
                        y[k] = gh;
                    }
                }
                __syncthreads();
                if (*bad) st = DAQP_BACKWARD_SINGULAR;
            }
            if (st == 0 && na > 0) {
                for (int e = tid; e < na * na; e += T) {
                    const int k = e / na, l = e - k * na;
                    if constexpr (SOFT) {
                        if (l == k && (side[k] & 2)) G[tri(k) + k] *= sn[k] * sn[k] * (1.0 + b.st.rho_soft);      // N_k N_k' + S_kk
                        else if (l <= k) G[tri(k) + l] *= sn[k] * sn[l];
                    } else {
                        if (l <= k) G[tri(k) + l] *= sn[k] * sn[l];
                    }
                }
                if constexpr (SOFT && DUAL) {      // N_W w - ghat_lamW
                    for (int k = tid; k < na; k += T) rhs[k] = (rhs[k] - y[k]) * sn[k];
                } else if constexpr (DUAL) {      // N_W w - g_lamW: the rows above are unscaled already, so sn is all that meets g_lam
                    const double *gl = a.grad_lam + (size_t)q * m;
                    for (int k = tid; k < na; k += T) rhs[k] = (rhs[k] - gl[ids[k]]) * sn[k];
                } else {
                    for (int k = tid; k < na; k += T) rhs[k] *= sn[k];
                }
                // ---- Cholesky in place (right-looking), diagonal in dg; a pivot below zero_tol ends it
                for (int c = 0; c < na; ++c) {
                    __syncthreads();
                    const double piv = G[tri(c) + c];
                    if (piv < b.st.zero_tol) { st = DAQP_BACKWARD_SINGULAR; break; }
                    const double d = sqrt(piv);
                    if (tid == 0) dg[c] = d;
                    for (int r = c + 1 + tid; r < na; r += T) G[tri(r) + c] /= d;
                    __syncthreads();
                    const int cnt = na - c - 1;
                    for (int e = tid; e < cnt * cnt; e += T) {
                        const int r0 = e / cnt, s0 = e - r0 * cnt;
                        if (s0 > r0) continue;
                        const int r = c + 1 + r0, s = c + 1 + s0;
                        G[tri(r) + s] -= G[tri(r) + c] * G[tri(s) + c];
                    }
                }
            }
            if (st == 0 && na > 0) {
                // ---- L y = rhs, L' z = y (z lands in rhs)
                for (int c = 0; c < na; ++c) {
                    __syncthreads();
                    const double yc = rhs[c] / dg[c];
                    if (tid == 0) y[c] = yc;
                    for (int r = c + 1 + tid; r < na; r += T) rhs[r] -= G[tri(r) + c] * yc;
                }
                for (int c = na - 1; c >= 0; --c) {
                    __syncthreads();
                    const double zc = y[c] / dg[c];
                    if (tid == 0) rhs[c] = zc;
                    for (int r = tid; r < c; r += T) y[r] -= G[tri(c) + r] * zc;
                }
                __syncthreads();
                for (int k = tid; k < na; k += T) y[k] = rhs[k] * sn[k];      // dnu
                __syncthreads();
                // ---- t = w - N_W' dnu (in gp)
                for (int j = tid; j < n; j += T) {
                    double s = w[j];
                    for (int k = 0; k < na; ++k) s -= Nr[(size_t)k * ldn + j] * y[k];
                    gp[j] = s;
                }
                for (int k = tid; k < na; k += T) ((SOFT ? (side[k] & 1) : side[k]) ? dbl : dbu)[ids[k]] = y[k];
                if constexpr (SOFT) {
                    if (a.usoft || a.usoft_id) {      // (block-uniform) u_k = R^-1 N_k' of the SOFT rows, in working-set order
                        int *slot = reinterpret_cast<int *>(dg);      // the Cholesky diagonal is spent: ns < cap ints fit
                        for (int s = tid; s < ns; s += T) slot[s] = -1;
                        __syncthreads();
                        for (int k = tid; k < na; k += T) {
                            if (!(side[k] & 2)) continue;
                            int cnt = 0;
                            for (int l = 0; l < k; ++l) cnt += (side[l] >> 1) & 1;
                            if (cnt < ns) slot[cnt] = k;
                        }
                        __syncthreads();
                        if (a.usoft_id) for (int s = tid; s < ns; s += T) { if (slot[s] >= 0) a.usoft_id[(size_t)q * ns + s] = ids[slot[s]]; }
                        if (a.usoft) {
                            double *uq = a.usoft + (size_t)q * ns * n;
                            if constexpr (RL) {
                                for (int e = tid; e < ns * n; e += T) {
                                    const int s = e / n, i = e - s * n, k = slot[s];
                                    if (k < 0) continue;
                                    const double *row = R + roff(i, n), *x1 = Nr + (size_t)k * ldn;
                                    double acc = 0;
                                    for (int j = i; j < n; ++j) acc += row[j] * x1[j];
                                    uq[e] = rs[i] * acc;
                                }
                            } else {      // a wave per element, as for dz below
                                const int lane = tid & 63;
                                for (int e = tid >> 6; e < ns * n; e += T / 64) {
                                    const int s = e / n, i = e - s * n, k = slot[s];
                                    if (k < 0) continue;      // (wave-uniform)
                                    const double *row = R + roff(i, n), *x1 = Nr + (size_t)k * ldn;
                                    double acc = 0;
                                    for (int j = i + lane; j < n; j += 64) acc += row[j] * x1[j];
                                    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
                                    if (lane == 0) uq[e] = rs[i] * acc;
                                }
                            }
                        }
                    }
                }
            } else if (st == 0) {
                for (int j = tid; j < n; j += T) gp[j] = w[j];
            }
            __syncthreads();
            // ---- dz = R^-1 t
            if (st == 0) {
                if constexpr (RL) {
                    for (int i = tid; i < n; i += T) {
                        const double *row = R + roff(i, n);
                        double s = 0;
                        for (int j = i; j < n; ++j) s += row[j] * gp[j];
                        dzq[i] = rs[i] * s;
                    }
                } else {      // a wave per row of R^-1 in HBM: coalesced, then a butterfly
                    const int lane = tid & 63;
                    for (int i = tid >> 6; i < n; i += T / 64) {
                        const double *row = R + roff(i, n);
                        double s = 0;
                        for (int j = i + lane; j < n; j += 64) s += row[j] * gp[j];
                        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
                        if (lane == 0) dzq[i] = rs[i] * s;
                    }
                }
            }
        }
        if (st != 0) for (int i = tid; i < n; i += T) dzq[i] = 0.0;
        if constexpr (SOFT) { if (st != 0 && a.qsoft) for (int r = tid; r < m; r += T) a.qsoft[(size_t)q * m + r] = 0.0; }
        if (tid == 0) a.status[q] = st;
        __syncthreads();      // the next problem of this workgroup reuses everything
    }
}

} // namespace daqp_amd
