// refine.hip.h -- fixed-precision iterative refinement of a solved batch at its stored working set.
//
// The solve runs in the least-distance coordinates u = R x + v and transforms back through the computed R^-1, so its (x, lam) carry an
// error of about cond(H) 2^-53.  At the stored working set W (rows C_W of C = [first ms rows of I; A], unsigned; b_W = bupper_k or
// blower_k by the DAQP_LOWER bit of the workspace's sense; lam signed) the optimum solves  H x + f + C_W' lam_W = 0,  C_W x = b_W.
// One step:
//
//     r1 = -(H x + f + C_W' lam_W),   r2 = b_W - C_W x          in twice the working precision (the pairs of certify.hip.h: products
//                                                               split with one fma, pairs summed across lanes, rounded ONCE), on the
//                                                               caller's own H, f, A, bupper, blower (BatchDev::H / f / A / bu / bl)
//     [ H    C_W' ] [ dx   ]   [ r1 ]
//     [ C_W  0    ] [ dlam ] = [ r2 ]                           in fp64 on the kept factor H = R'R -- the algebra of k_backward
//                                                               (backward.hip.h) with a non-zero second block:
//         w = R^-T r1,   N_W = C_W R^-1 (rows scaled to unit length),   (N_W N_W') dlam = N_W w - r2 (Cholesky),   dx = R^-1 (w - N_W' dlam)
//     x += dx,   lam_W += dlam
//
// N_W, its Gram matrix and the Cholesky factor do not depend on (x, lam): they are built once per problem and every step reuses them.
//
// Merit of a pair (the residuals are the doubled-precision ones):
//     mu = max( |r1|_inf / max(1, |Hx|_inf, |f|_inf, |C_W'|lam_W||_inf),   max_k |r2_k| / max(1, |b_k|, sum_j |c_kj x_j|) )
// A step is kept only if it lowers mu; the loop ends at the first step that does not (x, lam go back to what they were), at
// mu <= 2^-50, after a kept step that gained less than a factor 2, or after max_steps steps.  The pair that leaves never has a larger
// mu than the pair that came in.  NaN never compares smaller: a NaN anywhere leaves the inputs as they are.
//
// Status per problem: the rules of k_backward<.., SOFT = false> -- the setup / update / exit flag of a problem that did not end
// DAQP_EXIT_OPTIMAL, DAQP_EXIT_UNSUPPORTED after the proximal loop (the kept factor is that of H + eps I), DAQP_BACKWARD_SINGULAR when a
// pivot of the Gram Cholesky falls below zero_tol.  Such a problem's x and lam are not written, its residuals are NaN, its steps 0.
//
// What is read: Rinv, scaling, WS, QState, sense as k_backward reads them, and the caller's H, f, A and bounds in place.  Nothing of the
// batch is written.  How R^-1 is stored: backward.hip.h.
//
// Mapping: the tiers of k_backward.  One workgroup per problem, persistent over q, q + grid, ...; T = 64 (ONE wavefront; R^-1, the rows
// and the Gram matrix in LDS) while n <= 64; T = 256 beyond, R^-1 streamed from HBM, rows and Gram matrix in LDS where they fit (NL)
// and in a per-WORKGROUP scratch where they do not.  H and the active rows of A are streamed from HBM for every evaluation of the
// residuals: a wave per row for (Hx)_i and c_k x (lanes across columns, one pair butterfly per row), a thread per column for C_W' lam_W.
// No array lives in registers: every vector is in LDS (odd row stride for the rows, as in backward.hip.h).
#pragma once
#include "batch_dev.hip.h"
#include "certify.hip.h"

namespace daqp_amd {

struct RefineArgs {
    double *x, *lam;              // [N][n], [N][m]: in / out
    double *fval;                 // [N], or null
    double *residual;             // [N][2]: mu before, mu after; or null
    int *steps;                   // [N] kept steps, or null
    int *status;                  // [N]
    double *scratch;              // [grid][scratch_per_wg] (NL == false), or null
    size_t scratch_per_wg;
    int max_steps;
};

constexpr int kRefineMaxSteps = 8;
constexpr int kRefineRed = 16;      // doubles of LDS the block reductions go through

// LDS of one workgroup in bytes: rs, gp, w, xc, xp, r1 (n each), rhs, y, sn, dg, lc, lp, r2 (cap each), the reduction words, then
// R^-1 (RL), rows + Gram (NL), ids, side, flag
__host__ __device__ inline size_t refine_lds_bytes(int n, int cap, bool rl, bool nl)
{
    size_t dbl = 6 * (size_t)n + 7 * (size_t)cap + kRefineRed;
    if (rl) dbl += (size_t)n * (n + 1) / 2;
    if (nl) dbl += (size_t)cap * (n | 1) + (size_t)tri(cap);
    return dbl * sizeof(double) + (2 * (size_t)cap + 2) * sizeof(int);
}
__host__ __device__ inline size_t refine_scratch_doubles(int n, int cap) { return (size_t)cap * (n | 1) + (size_t)tri(cap); }

// the same value in every thread of the block; NaN is never dropped
template <int T>
__device__ __forceinline__ double rf_block_max(double v, double *red)
{
    v = cert_wave_nanmax(v);
    if constexpr (T > 64) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        __syncthreads();
        if (lane == 0) red[wave] = v;
        __syncthreads();
        v = red[0];
        for (int w = 1; w < T / 64; ++w) v = cert_nanmax(v, red[w]);
    }
    return v;
}
// pairs, waves added in wave order
template <int T>
__device__ __forceinline__ dd rf_block_sum(dd v, double *red)
{
    v = dd_wave_sum(v, 64, 1);
    if constexpr (T > 64) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        __syncthreads();
        if (lane == 0) { red[2 * wave] = v.hi; red[2 * wave + 1] = v.lo; }
        __syncthreads();
        v = {red[0], red[1]};
        for (int w = 1; w < T / 64; ++w) dd_acc(v, dd{red[2 * w], red[2 * w + 1]});
    }
    return v;
}

// one problem's data and the LDS vectors an evaluation reads and writes
struct RefineCtx {
    int n, ms, na;
    const double *H, *f, *A, *bu, *bl;      // HBM, this problem's
    const double *xc, *lc;                  // the pair: x [n], lam on W [na]
    double *hh, *hl;                        // (Hx)_i as pairs [n] each
    double *r1, *r2, *red;
    const int *ids, *side;
};

// r1, r2 (rounded once from pairs), mu and 1/2 x'Hx + f'x of the pair in c.xc, c.lc; mu and obj are block-uniform.  Ends behind a
// barrier: r1 and r2 are there for every thread.
template <int T>
__device__ __forceinline__ void rf_eval(const RefineCtx &c, double &mu, double &obj)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = c.n;
    // ---- (Hx)_i: a wave per row of H
    for (int i = wave; i < n; i += T / 64) {
        const double *row = c.H + (size_t)i * n;
        dd part = {0.0, 0.0};
        for (int j = lane; j < n; j += 64) dd_acc(part, dd_two_prod(row[j], c.xc[j]));
        const dd hx = dd_wave_sum(part, 64, 1);
        if (lane == 0) { c.hh[i] = hx.hi; c.hl[i] = hx.lo; }
    }
    // ---- r2_k = b_k - c_k x: a wave per row of W
    double rmax = 0.0;
    for (int k = wave; k < c.na; k += T / 64) {
        const int id = c.ids[k];
        dd cx;
        double ax;
        if (id < c.ms) { cx = {c.xc[id], 0.0}; ax = fabs(c.xc[id]); }
        else {
            const double *row = c.A + (size_t)(id - c.ms) * n;
            dd part = {0.0, 0.0};
            double pa = 0.0;
            for (int j = lane; j < n; j += 64) {
                const dd t = dd_two_prod(row[j], c.xc[j]);
                dd_acc(part, t);
                pa += fabs(t.hi);
            }
            cx = dd_wave_sum(part, 64, 1);
            for (int o = 32; o > 0; o >>= 1) pa += __shfl_xor(pa, o, 64);
            ax = pa;
        }
        const double bk = c.side[k] ? c.bl[id] : c.bu[id];
        const dd s = dd_two_sum(bk, -cx.hi);
        const double r = s.hi + (s.lo - cx.lo);
        if (lane == 0) c.r2[k] = r;
        rmax = cert_nanmax(rmax, fabs(r) / cert_nanmax(cert_nanmax(1.0, fabs(bk)), ax));
    }
    __syncthreads();
    // ---- r1_j = -((Hx)_j + f_j + (C_W' lam_W)_j): a thread per column
    double m_r1 = 0.0, m_hx = 0.0, m_f = 0.0, m_cl = 0.0;
    dd ob = {0.0, 0.0};
    for (int j = tid; j < n; j += T) {
        const dd hx = {c.hh[j], c.hl[j]};
        const double fj = c.f[j], xj = c.xc[j];
        dd acc = hx, cl = {0.0, 0.0};
        dd_acc(acc, fj);
        for (int k = 0; k < c.na; ++k) {
            const int id = c.ids[k];
            const double lk = c.lc[k];
            if (id < c.ms) {
                if (id == j) { dd_acc(acc, lk); dd_acc(cl, fabs(lk)); }
            } else {
                const double av = c.A[(size_t)(id - c.ms) * n + j];
                dd_acc(acc, dd_two_prod(av, lk));
                dd_acc(cl, dd_two_prod(av, fabs(lk)));
            }
        }
        const double r = -dd_round(acc);
        c.r1[j] = r;
        m_r1 = cert_nanmax(m_r1, fabs(r));
        m_hx = cert_nanmax(m_hx, fabs(dd_round(hx)));
        m_f = cert_nanmax(m_f, fabs(fj));
        m_cl = cert_nanmax(m_cl, fabs(dd_round(cl)));
        dd t = dd_two_prod(hx.hi, 0.5 * xj);
        t.lo += hx.lo * (0.5 * xj);
        dd_acc(ob, t);
        dd_acc(ob, dd_two_prod(fj, xj));
    }
    m_r1 = rf_block_max<T>(m_r1, c.red);
    m_hx = rf_block_max<T>(m_hx, c.red);
    m_f = rf_block_max<T>(m_f, c.red);
    m_cl = rf_block_max<T>(m_cl, c.red);
    rmax = rf_block_max<T>(rmax, c.red);
    obj = dd_round(rf_block_sum<T>(ob, c.red));
    mu = cert_nanmax(m_r1 / cert_nanmax(cert_nanmax(1.0, m_hx), cert_nanmax(m_f, m_cl)), rmax);
    __syncthreads();
}

template <int T, bool RL, bool NL>
__global__ __launch_bounds__(T) void k_refine(BatchDev b, RefineArgs a)
{
    extern __shared__ double lds_rf[];
    const int tid = threadIdx.x, n = b.n, m = b.m, ms = b.ms, cap = b.cap, mA = b.mA;
    const int ldn = n | 1;      // odd row stride: the Gram dot products walk several rows at once
    double *rs = lds_rf, *gp = rs + n, *w = gp + n, *xc = w + n, *xp = xc + n, *r1 = xp + n;
    double *rhs = r1 + n, *y = rhs + cap, *sn = y + cap, *dg = sn + cap, *lc = dg + cap, *lp = lc + cap, *r2 = lp + cap, *red = r2 + cap;
    double *p = red + kRefineRed;
    double *Rl = nullptr, *Nr, *G;
    if constexpr (RL) { Rl = p; p += b.rtri; }
    if constexpr (NL) { Nr = p; p += (size_t)cap * ldn; G = p; p += tri(cap); }
    else { Nr = a.scratch + (size_t)blockIdx.x * a.scratch_per_wg; G = Nr + (size_t)cap * ldn; }
    int *ids = reinterpret_cast<int *>(p), *side = ids + cap, *bad = side + cap;

    for (int q = blockIdx.x; q < b.N; q += gridDim.x) {
        const QState *qs = b.qs + q;
        double *xq = a.x + (size_t)q * n, *lq = a.lam + (size_t)q * m;
        // ---- what the solve left: every read below is block-uniform
        int st = 0, na = qs->n_active;
        {
            const int sflag = qs->setup_flag, uflag = qs->upd_flag, eflag = qs->exitflag;
            if (sflag < 0) st = sflag;
            else if (uflag < 0) st = uflag;
            else if (eflag != DAQP_EXIT_OPTIMAL) st = eflag != 0 ? eflag : DAQP_EXIT_UNSUPPORTED;
            else if (qs->n_prox > 0) st = DAQP_EXIT_UNSUPPORTED;
            else if (qs->sing_ind == DAQP_UNCONSTRAINED_OPTIMAL) na = 0;      // the shortcut: W is empty
            if (st == 0 && (na < 0 || na > cap)) st = DAQP_BACKWARD_SINGULAR;
        }
        double mu_in = 0.0, mu = 0.0, obj = 0.0;
        int kept = 0;
        if (st == 0) {
            const size_t qF = qf(b, q);
            const double *Rg = b.Rinv + qF * b.rtri, *sc = b.scaling + qF * m;
            const double *Aq = b.A + (b.shared ? qF : (size_t)q) * mA * n;
            const double *R = Rg;
            if constexpr (RL) { for (int e = tid; e < b.rtri; e += T) Rl[e] = Rg[e]; R = Rl; }
            const int diag = qs->diag_h;
            if (tid == 0) *bad = 0;
            for (int i = tid; i < n; i += T) {
                rs[i] = (i < ms && !diag) ? 1.0 / sc[i] : 1.0;
                xc[i] = xq[i];
            }
            __syncthreads();
            for (int k = tid; k < na; k += T) {
                const int id = b.WS[(size_t)q * cap + k];
                if (id < 0 || id >= m) { ids[k] = 0; side[k] = 0; lc[k] = 0.0; *bad = 1; }
                else {
                    ids[k] = id;
                    side[k] = (b.sense[(size_t)q * m + id] & DAQP_LOWER) ? 1 : 0;
                    lc[k] = lq[id];
                }
            }
            __syncthreads();
            if (*bad) st = DAQP_BACKWARD_SINGULAR;
            // ---- rows of N_W = C_W R^-1 (unscaled), their Gram matrix (packed lower), its Cholesky factor: once per problem
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
                for (int e = tid; e < na * na; e += T) {
                    const int k = e / na, l = e - k * na;
                    if (l > k) continue;
                    const double *x1 = Nr + (size_t)k * ldn, *x2 = Nr + (size_t)l * ldn;
                    double s = 0;
                    for (int j = 0; j < n; ++j) s += x1[j] * x2[j];
                    G[tri(k) + l] = s;
                }
                __syncthreads();
                // rows to unit length: G <- S G S (dlam = S * the solution of the scaled system)
                for (int k = tid; k < na; k += T) {
                    const double d = G[tri(k) + k];
                    if (!(d > 0.0)) { sn[k] = 0.0; *bad = 1; } else sn[k] = 1.0 / sqrt(d);
                }
                __syncthreads();
                if (*bad) st = DAQP_BACKWARD_SINGULAR;
            }
            if (st == 0 && na > 0) {
                for (int e = tid; e < na * na; e += T) {
                    const int k = e / na, l = e - k * na;
                    if (l <= k) G[tri(k) + l] *= sn[k] * sn[l];
                }
                // Cholesky in place (right-looking), diagonal in dg; a pivot below zero_tol ends it
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
            __syncthreads();
            if (st == 0) {
                RefineCtx c;
                c.n = n; c.ms = ms; c.na = na;
                c.H = b.H + qF * (size_t)n * n; c.f = b.f + (size_t)q * n; c.A = Aq;
                c.bu = b.bu + (size_t)q * m; c.bl = b.bl + (size_t)q * m;
                c.xc = xc; c.lc = lc; c.hh = gp; c.hl = w; c.r1 = r1; c.r2 = r2; c.red = red; c.ids = ids; c.side = side;
                rf_eval<T>(c, mu, obj);
                mu_in = mu;
                // (mu, kept: block-uniform -- every branch below is taken by the whole workgroup)
                while (kept < a.max_steps && mu > 0x1p-50) {
                    const double mu_p = mu, obj_p = obj;
                    for (int i = tid; i < n; i += T) { xp[i] = xc[i]; gp[i] = r1[i] * rs[i]; }
                    for (int k = tid; k < na; k += T) lp[k] = lc[k];
                    __syncthreads();
                    // ---- w = R^-T r1
                    for (int j = tid; j < n; j += T) {
                        double s = 0;
                        for (int i = 0; i <= j; ++i) s += R[roff(i, n) + j] * gp[i];
                        w[j] = s;
                    }
                    __syncthreads();
                    if (na > 0) {
                        for (int k = tid; k < na; k += T) {
                            const double *x1 = Nr + (size_t)k * ldn;
                            double s = 0;
                            for (int j = 0; j < n; ++j) s += x1[j] * w[j];
                            rhs[k] = (s - r2[k]) * sn[k];
                        }
                        // L y = rhs, L' z = y (z lands in rhs)
                        for (int cc = 0; cc < na; ++cc) {
                            __syncthreads();
                            const double yc = rhs[cc] / dg[cc];
                            if (tid == 0) y[cc] = yc;
                            for (int r = cc + 1 + tid; r < na; r += T) rhs[r] -= G[tri(r) + cc] * yc;
                        }
                        for (int cc = na - 1; cc >= 0; --cc) {
                            __syncthreads();
                            const double zc = y[cc] / dg[cc];
                            if (tid == 0) rhs[cc] = zc;
                            for (int r = tid; r < cc; r += T) y[r] -= G[tri(cc) + r] * zc;
                        }
                        __syncthreads();
                        for (int k = tid; k < na; k += T) y[k] = rhs[k] * sn[k];      // dlam
                        __syncthreads();
                        // t = w - N_W' dlam (in gp)
                        for (int j = tid; j < n; j += T) {
                            double s = w[j];
                            for (int k = 0; k < na; ++k) s -= Nr[(size_t)k * ldn + j] * y[k];
                            gp[j] = s;
                        }
                        for (int k = tid; k < na; k += T) lc[k] += y[k];
                    } else {
                        for (int j = tid; j < n; j += T) gp[j] = w[j];
                    }
                    __syncthreads();
                    // ---- x += R^-1 t
                    if constexpr (RL) {
                        for (int i = tid; i < n; i += T) {
                            const double *row = R + roff(i, n);
                            double s = 0;
                            for (int j = i; j < n; ++j) s += row[j] * gp[j];
                            xc[i] += rs[i] * s;
                        }
                    } else {      // a wave per row of R^-1 in HBM: coalesced, then a butterfly
                        const int lane = tid & 63;
                        for (int i = tid >> 6; i < n; i += T / 64) {
                            const double *row = R + roff(i, n);
                            double s = 0;
                            for (int j = i + lane; j < n; j += 64) s += row[j] * gp[j];
                            for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
                            if (lane == 0) xc[i] += rs[i] * s;
                        }
                    }
                    __syncthreads();
                    rf_eval<T>(c, mu, obj);
                    if (!(mu < mu_p)) {      // rejected: the pair goes back to what it was
                        for (int i = tid; i < n; i += T) xc[i] = xp[i];
                        for (int k = tid; k < na; k += T) lc[k] = lp[k];
                        mu = mu_p; obj = obj_p;
                        break;
                    }
                    ++kept;
                    if (!(mu <= 0.5 * mu_p)) break;      // kept, but it gained less than a factor 2
                }
                __syncthreads();
                for (int i = tid; i < n; i += T) xq[i] = xc[i];
                for (int r = tid; r < m; r += T) lq[r] = 0.0;
                __syncthreads();
                for (int k = tid; k < na; k += T) lq[ids[k]] = lc[k];
            }
        }
        if (tid == 0) {
            const double nan = __longlong_as_double(0x7ff8000000000000LL);
            a.status[q] = st;
            if (a.steps) a.steps[q] = st == 0 ? kept : 0;
            if (a.residual) { a.residual[2 * (size_t)q] = st == 0 ? mu_in : nan; a.residual[2 * (size_t)q + 1] = st == 0 ? mu : nan; }
            if (a.fval && st == 0) a.fval[q] = obj;
        }
        __syncthreads();      // the next problem of this workgroup reuses everything
    }
}

extern template __global__ void k_refine<64, true, true>(BatchDev, RefineArgs);
extern template __global__ void k_refine<256, false, true>(BatchDev, RefineArgs);
extern template __global__ void k_refine<256, false, false>(BatchDev, RefineArgs);

} // namespace daqp_amd
