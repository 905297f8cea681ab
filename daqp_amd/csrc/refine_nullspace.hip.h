// refine_nullspace.hip.h -- iterative refinement of a solved batch at its stored working set WITHOUT a factor of H: the step of
// refine.hip.h solved by the null-space method of nullspace.hip.h on the caller's own Hessian.
//
// k_refine solves the correction on the kept factor H = R'R, so a problem that went through the proximal loop (singular H, an LP)
// -- whose kept factor is that of H + eps I -- gets DAQP_EXIT_UNSUPPORTED from it.  Those are the problems whose (x, lam) are limited by
// the outer fixed-point tolerance eta_prox / eps and not by the arithmetic.  The system of one step,
//
//     [ H    C_W' ] [ dx   ]   [ r1 ]        r1 = -(H x + f + C_W' lam_W)
//     [ C_W  0    ] [ dlam ] = [ r2 ]        r2 = b_W - C_W x
//
// is nonsingular whenever the optimum is locally unique, and is solved here as k_backward_nullspace solves its own:
//
//     once per problem (steps 1 - 3 of nullspace.hip.h, restated: that kernel is not touched)
//         rows     the k = n_active rows of C_W scaled to unit length, the norms s kept
//         QR       C_W' = Q [R; 0], Householder, left-looking;  R_jj^2 < zero_tol  is DAQP_BACKWARD_SINGULAR
//         Hr       Z'HZ (Z = the last n - k columns of Q) and its Cholesky factor; a pivot <= zero_tol max(1, max_i H_ii) is
//                  DAQP_BACKWARD_SINGULAR.  An LP has H = 0: anything but a vertex (k = n) is singular
//     per step, fp64
//         y  = R^-T (r2 / s)                       (k entries)
//         t  = r1 - H Q [y; 0]
//         z  = Hr^-1 (Q't)[k:]                     (n - k entries; none at a vertex)
//         dx = Q [y; z]
//         dlam = R^-1 (Q'(r1 - H dx))[:k] / s
//         x += dx,  lam_W += dlam
//
// The residuals, the merit mu and 1/2 x'Hx + f'x of a pair come from ONE evaluation in twice the working precision (the pairs of
// certify.hip.h: products split with one fma, pairs summed, rounded once), as rf_eval of refine.hip.h forms them; the merit, the
// acceptance rule and the end conditions are those of refine.hip.h word for word: a step is kept only if it lowers mu; the loop ends
// at the first rejected step, at mu <= 2^-50, after a kept step that gained less than a factor 2, or after max_steps steps.  The pair
// that leaves never has a larger mu than the pair that came in; a NaN anywhere leaves the inputs as they are.
//
// Status per problem: the rules of k_backward_nullspace.  With a non-zero status x, lam and fval are not written, steps is 0 and
// both residuals are NaN.
//
// What is read: WS, QState, sense, and the caller's H, f, A, bupper, blower in place (BatchDev::H / f / A / bu / bl; H through qf() for
// shared batches) -- adopted device arrays must still be valid at the call.  H is taken symmetric.  An LP batch holds ONE identity
// matrix in BatchDev::H: lp != 0 says H = 0.  Rinv, scaling, L, vecs and Mblk are NOT read; nothing of the batch is written.
//
// Mapping: that of k_backward_nullspace.  One wavefront per problem, n <= 64; lane i owns element i of every n-vector and row i of W
// (its id, side, bound, multiplier and r2 -- k <= n), all in registers; LDS holds the reflectors with R above them, Hr behind them and
// three n-vectors: nullspace_lds_bytes(n), 34.8 KB at n = 64.  (H x)_i and c_i x are walked by lane i (H by columns, which the lanes
// read side by side) and C_W' lam_W by lane j over the rows: no evaluation needs a reduction of pairs but the objective's.
#pragma once
#include "nullspace.hip.h"
#include "refine.hip.h"

namespace daqp_amd {

struct RefineNullspaceArgs {
    RefineArgs r;                   // x, lam, fval, residual, steps, status, max_steps as k_refine takes them (scratch unused)
    int lp;                         // the batch is an LP batch: b.H is the setup's identity, H = 0
    int only_prox;                  // 1: only the problems with n_prox > 0 (the others were written by k_refine and stay untouched)
};

// r1 (element `lane`), r2 (row `lane` of W), mu and 1/2 x'Hx + f'x of the pair (x, lam): x is element `lane` (zero in the lanes >= n),
// lam, id, bk belong to row `lane` of W (lanes < k).  mu and obj are the same in every lane.
__device__ __forceinline__ void rns_eval(const double *H, const double *fq, const double *Aq, int n, int ms, int k, int lp, int lane, int id,
                                         double bk, double x, double lam, double &r1, double &r2, double &mu, double &obj)
{
    // ---- (H x)_i: lane i walks column i of the symmetric H
    dd hx = {0.0, 0.0};
    if (!lp) {
        for (int l = 0; l < n; ++l) {
            const double xl = __shfl(x, l, 64);
            if (lane < n) dd_acc(hx, dd_two_prod(H[(size_t)l * n + lane], xl));
        }
    }
    // ---- r2_c = b_c - c_c x: lane c walks row c of W
    dd cx = {0.0, 0.0};
    double ax = 0.0;
    for (int j = 0; j < n; ++j) {
        const double xj = __shfl(x, j, 64);
        if (lane < k) {
            if (id < ms) { if (id == j) { cx = {xj, 0.0}; ax = fabs(xj); } }
            else {
                const dd t = dd_two_prod(Aq[(size_t)(id - ms) * n + j], xj);
                dd_acc(cx, t);
                ax += fabs(t.hi);
            }
        }
    }
    double rmax = 0.0;
    r2 = 0.0;
    if (lane < k) {
        const dd s = dd_two_sum(bk, -cx.hi);
        r2 = s.hi + (s.lo - cx.lo);
        rmax = fabs(r2) / cert_nanmax(cert_nanmax(1.0, fabs(bk)), ax);
    }
    rmax = cert_wave_nanmax(rmax);
    // ---- r1_j = -((Hx)_j + f_j + (C_W' lam_W)_j): lane j walks the rows of W
    const double fj = lane < n ? fq[lane] : 0.0;
    dd acc = hx, cl = {0.0, 0.0};
    dd_acc(acc, fj);
    for (int c = 0; c < k; ++c) {
        const int idc = __shfl(id, c, 64);
        const double lc = __shfl(lam, c, 64);
        if (idc < ms) {
            if (idc == lane) { dd_acc(acc, lc); dd_acc(cl, fabs(lc)); }
        } else if (lane < n) {
            const double av = Aq[(size_t)(idc - ms) * n + lane];
            dd_acc(acc, dd_two_prod(av, lc));
            dd_acc(cl, dd_two_prod(av, fabs(lc)));
        }
    }
    r1 = lane < n ? -dd_round(acc) : 0.0;
    const double m_r1 = cert_wave_nanmax(fabs(r1));
    const double m_hx = cert_wave_nanmax(fabs(dd_round(hx)));
    const double m_f = cert_wave_nanmax(fabs(fj));
    const double m_cl = cert_wave_nanmax(lane < n ? fabs(dd_round(cl)) : 0.0);
    dd ob = dd_two_prod(hx.hi, 0.5 * x);
    ob.lo += hx.lo * (0.5 * x);
    dd_acc(ob, dd_two_prod(fj, x));
    obj = dd_round(dd_wave_sum(ob, 64, 1));
    mu = cert_nanmax(m_r1 / cert_nanmax(cert_nanmax(1.0, m_hx), cert_nanmax(m_f, m_cl)), rmax);
}

// (a template only so that refine_kernel.hip holds the one instantiation: T is the wavefront, 64)
template <int T>
__global__ __launch_bounds__(T) void k_refine_nullspace(BatchDev b, RefineNullspaceArgs a)
{
    static_assert(T == 64, "one wavefront per problem");
    extern __shared__ double lds_rns[];
    const int lane = threadIdx.x, n = b.n, m = b.m, ms = b.ms, cap = b.cap, mA = b.mA;
    const int q = blockIdx.x;
    if (q >= b.N || n > 64) return;
    const QState *qs = b.qs + q;
    if (a.only_prox && !(qs->n_prox > 0)) return;      // (block-uniform)
    const int ldn = n | 1;
    double *V = lds_rns, *beta = V + (size_t)n * ldn, *rd = beta + n, *rn = rd + n;
    // ---- what the solve left: every read below is block-uniform
    int st = 0, k = qs->n_active;
    {
        const int sflag = qs->setup_flag, uflag = qs->upd_flag, eflag = qs->exitflag;
        if (sflag < 0) st = sflag;
        else if (uflag < 0) st = uflag;
        else if (eflag != DAQP_EXIT_OPTIMAL) st = eflag != 0 ? eflag : DAQP_EXIT_UNSUPPORTED;
        else if (qs->sing_ind == DAQP_UNCONSTRAINED_OPTIMAL) k = 0;      // the shortcut: W is empty
        if (st == 0 && (k < 0 || k > n || k > cap)) st = DAQP_BACKWARD_SINGULAR;      // (more than n rows are linearly dependent)
    }
    const size_t qF = qf(b, q);
    const double *H = b.H + qF * (size_t)n * n;
    const double *Aq = b.A + (b.shared ? qF : (size_t)q) * mA * n;
    const double *fq = b.f + (size_t)q * n;
    const int nz = n - k, ldz = nz | 1;
    double *Hr = V + (size_t)k * ldn;      // element (r, c), r >= c, at Hr[c * ldz + r]
    double *xq = a.r.x + (size_t)q * n, *lq = a.r.lam + (size_t)q * m;

    // ---- row `lane` of W: its id, its bound by the DAQP_LOWER bit, its multiplier
    int id = 0;
    double bk = 0.0, lam = 0.0;
    if (st == 0) {
        int bad = 0;
        if (lane < k) {
            id = b.WS[(size_t)q * cap + lane];
            if (id < 0 || id >= m) { bad = 1; id = 0; }
            else {
                const int sg = b.sense[(size_t)q * m + id];
                bk = ((sg & DAQP_LOWER) ? b.bl : b.bu)[(size_t)q * m + id];
                lam = lq[id];
            }
        }
        if (__any(bad)) st = DAQP_BACKWARD_SINGULAR;
    }

    // ---- 1, 2: the rows of C_W, unit length, and the QR of C_W' one column at a time
    for (int c = 0; st == 0 && c < k; ++c) {
        const int idc = __shfl(id, c, 64);
        double x = 0.0;
        if (lane < n) x = (idc < ms) ? (lane == idc ? 1.0 : 0.0) : Aq[(size_t)(idc - ms) * n + lane];
        const double len2 = ns_wsum(x * x);
        if (!(len2 > 0.0)) { st = DAQP_BACKWARD_SINGULAR; break; }
        const double len = sqrt(len2);
        x /= len;
        for (int j = 0; j < c; ++j) x = ns_reflect(x, V, beta, j, ldn, lane, n);
        const double sigma = ns_wsum(lane >= c ? x * x : 0.0);      // R_cc^2
        if (!(sigma >= b.st.zero_tol)) { st = DAQP_BACKWARD_SINGULAR; break; }
        const double alpha = __shfl(x, c, 64);
        const double rcc = alpha >= 0.0 ? -sqrt(sigma) : sqrt(sigma);
        const double u0 = alpha - rcc;      // (|u0| >= |R_cc| > 0)
        if (lane < n) V[(size_t)c * ldn + lane] = lane < c ? x : (lane == c ? 1.0 : x / u0);
        if (lane == 0) { beta[c] = -u0 / rcc; rd[c] = rcc; rn[c] = len; }
        __syncthreads();
    }

    // ---- 3: Hr = Z'HZ and its Cholesky factor
    if (st == 0 && nz > 0 && a.lp) st = DAQP_BACKWARD_SINGULAR;      // H = 0: every pivot of Hr is zero
    if (st == 0 && nz > 0) {
        const double hmax = ns_wmax(lane < n ? H[(size_t)lane * n + lane] : 0.0);
        const double tol = b.st.zero_tol * fmax(1.0, hmax);
        for (int j = 0; j < nz; ++j) {
            double z = lane == k + j ? 1.0 : 0.0;
            for (int c = k - 1; c >= 0; --c) z = ns_reflect(z, V, beta, c, ldn, lane, n);
            double t = ns_hmul(H, z, lane, n, 0);
            for (int c = 0; c < k; ++c) t = ns_reflect(t, V, beta, c, ldn, lane, n);
            if (lane >= k + j && lane < n) Hr[(size_t)j * ldz + (lane - k)] = t;      // the lower triangle is all the factorisation reads
        }
        __syncthreads();
        for (int c = 0; c < nz; ++c) {      // right-looking, lane r owns row r
            const double piv = Hr[(size_t)c * ldz + c];
            if (!(piv > tol)) { st = DAQP_BACKWARD_SINGULAR; break; }
            const double d = sqrt(piv);
            double lrc = 0.0;
            if (lane > c && lane < nz) lrc = Hr[(size_t)c * ldz + lane] / d;
            __syncthreads();
            if (lane > c && lane < nz) Hr[(size_t)c * ldz + lane] = lrc;
            if (lane == c) Hr[(size_t)c * ldz + c] = d;
            __syncthreads();
            for (int s = c + 1; s < nz; ++s) {
                const double lsc = Hr[(size_t)c * ldz + s];
                if (lane >= s && lane < nz) Hr[(size_t)s * ldz + lane] -= lrc * lsc;
            }
            __syncthreads();
        }
    }

    // ---- the steps: every branch below is taken by the whole wavefront (st, k, mu, kept are uniform)
    double mu_in = 0.0, mu = 0.0, obj = 0.0;
    int kept = 0;
    if (st == 0) {
        const double sc = lane < k ? rn[lane] : 1.0;
        double x = lane < n ? xq[lane] : 0.0;
        double r1, r2;
        rns_eval(H, fq, Aq, n, ms, k, a.lp, lane, id, bk, x, lam, r1, r2, mu, obj);
        mu_in = mu;
        while (kept < a.r.max_steps && mu > 0x1p-50) {
            const double mu_p = mu, obj_p = obj, xp = x, lamp = lam;
            // y = R^-T (r2 / s), lane i owns entry i
            double y = lane < k ? r2 / sc : 0.0;
            for (int c = 0; c < k; ++c) {
                const double yc = __shfl(y, c, 64) / rd[c];
                if (lane == c) y = yc;
                else if (lane > c && lane < k) y -= V[(size_t)lane * ldn + c] * yc;
            }
            double w = y;      // [y; z]
            if (nz > 0) {
                // t = r1 - H Q [y; 0], then z = Hr^-1 (Q't)[k:]
                double p = y;
                for (int c = k - 1; c >= 0; --c) p = ns_reflect(p, V, beta, c, ldn, lane, n);
                double t = r1 - ns_hmul(H, p, lane, n, 0);
                for (int c = 0; c < k; ++c) t = ns_reflect(t, V, beta, c, ldn, lane, n);
                double rhs = __shfl(t, (lane + k) & 63, 64);      // lane r < nz takes entry k + r
                if (lane >= nz) rhs = 0.0;
                for (int c = 0; c < nz; ++c) {      // L y1 = rhs
                    const double yc = __shfl(rhs, c, 64) / Hr[(size_t)c * ldz + c];
                    if (lane == c) rhs = yc;
                    else if (lane > c && lane < nz) rhs -= Hr[(size_t)c * ldz + lane] * yc;
                }
                for (int c = nz - 1; c >= 0; --c) {      // L' y2 = y1
                    const double yc = __shfl(rhs, c, 64) / Hr[(size_t)c * ldz + c];
                    if (lane == c) rhs = yc;
                    else if (lane < c) rhs -= Hr[(size_t)lane * ldz + c] * yc;
                }
                const double z = __shfl(rhs, (lane - k) & 63, 64);      // back to entry k + r of an n-vector
                if (lane >= k && lane < n) w = z;
            }
            double dx = w;
            for (int c = k - 1; c >= 0; --c) dx = ns_reflect(dx, V, beta, c, ldn, lane, n);
            if (k > 0) {
                double v = r1 - ns_hmul(H, dx, lane, n, a.lp);
                for (int c = 0; c < k; ++c) v = ns_reflect(v, V, beta, c, ldn, lane, n);
                for (int c = k - 1; c >= 0; --c) {      // R dlam~ = v(0 : k), lane i owns row i
                    const double dc = __shfl(v, c, 64) / rd[c];
                    if (lane == c) v = dc;
                    else if (lane < c) v -= V[(size_t)c * ldn + lane] * dc;
                }
                if (lane < k) lam += v / sc;
            }
            x += dx;
            rns_eval(H, fq, Aq, n, ms, k, a.lp, lane, id, bk, x, lam, r1, r2, mu, obj);
            if (!(mu < mu_p)) {      // rejected: the pair goes back to what it was
                x = xp; lam = lamp; mu = mu_p; obj = obj_p;
                break;
            }
            ++kept;
            if (!(mu <= 0.5 * mu_p)) break;      // kept, but it gained less than a factor 2
        }
        if (lane < n) xq[lane] = x;
        for (int r = lane; r < m; r += 64) lq[r] = 0.0;
        __syncthreads();
        if (lane < k) lq[id] = lam;
    }
    if (lane == 0) {
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        a.r.status[q] = st;
        if (a.r.steps) a.r.steps[q] = st == 0 ? kept : 0;
        if (a.r.residual) { a.r.residual[2 * (size_t)q] = st == 0 ? mu_in : nan; a.r.residual[2 * (size_t)q + 1] = st == 0 ? mu : nan; }
        if (a.r.fval && st == 0) a.r.fval[q] = obj;
    }
}

extern template __global__ void k_refine_nullspace<64>(BatchDev, RefineNullspaceArgs);

} // namespace daqp_amd
