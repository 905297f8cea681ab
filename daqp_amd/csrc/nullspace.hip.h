// nullspace.hip.h -- the adjoint of a solved batch WITHOUT a factor of H: the null-space method on the caller's own Hessian.
//
// The same system as backward.hip.h, at the stored working set W (rows C_W of C = [first ms rows of I; A], unsigned):
//
//     [ H    C_W' ] [ dz  ]   [ g ]
//     [ C_W  0    ] [ dnu ] = [ 0 ]
//
// k_backward solves it on the kept factor H = R'R.  A problem that went through the proximal loop (singular H, an LP) keeps the
// factor of H + eps I, not of H, and H itself may have no factor at all.  The system is still nonsingular whenever the optimum is
// locally unique -- C_W of full row rank, Z'HZ positive definite on the null space of C_W -- and that is all this kernel asks for:
//
//     1. rows      the k = n_active rows of C_W in the caller's units (a simple bound i < ms is e_i, a general row is A_i), each scaled
//                  to unit length, its norm kept
//     2. QR        Householder QR of C_W' (n x k), no pivoting, left-looking: C_W' = Q [R; 0].  R_jj^2 is the squared length of what
//                  is left of unit row j after the rows before it are projected out -- the pivot the Gram Cholesky of k_backward meets
//                  on its unit rows -- and  R_jj^2 < zero_tol  is DAQP_BACKWARD_SINGULAR as there.  More than n rows are dependent.
//     3. Hr        Z'HZ, Z = the last n - k columns of Q, column by column: z = Q e_(k+j), t = H z, the last n - k entries of Q't;
//                  Cholesky in place; a pivot <= zero_tol max(1, max_i H_ii) is DAQP_BACKWARD_SINGULAR (H not positive definite on
//                  the null space: the optimum is not locally unique).  An LP has H = 0: every pivot is zero, so k < n is singular
//                  and k = n (a vertex) has an empty Z and dz = 0.
//     4. solve     dz = Z Hr^-1 Z'g,   R dnu~ = Q1'(g - H dz),   dnu = dnu~ / |row|,   scattered to dbupper / dblower by the row's
//                  DAQP_LOWER bit exactly as k_backward does
//
// A dual right-hand side (DUAL == true: daqp_batch_backward_dual): K [dz; dnu] = [g; g_lamW], g_lamW[c] = grad_lam[WS[c]] the gradient
// with respect to the signed multipliers.  Steps 1 - 3 and both singularity tests are unchanged; step 4 becomes the step algebra of
// refine_nullspace.hip.h with r1 = g, r2 = g_lamW (s = the norms of the rows):
//     y = R^-T (g_lamW / s),   z = Hr^-1 (Q'(g - H Q [y; 0]))[k:],   dz = Q [y; z],   dnu = R^-1 (Q'(g - H dz))[:k] / s
// At an LP vertex (k = n) dz = Q y is no longer zero.  grad_x may be null (= 0).  DUAL == false compiles to what the kernel was.
//
// The system does not contain x or lam: the result depends on H, A and W only, not on how tightly the proximal loop converged.
//
// What is read: WS, QState, sense, A as k_backward reads them, and the caller's H through BatchDev::H (indexed with qf() for shared
// batches) -- adopted device arrays must therefore still be valid at the call.  H is taken symmetric (lane i walks column i, which
// the lanes of a wavefront read side by side).  An LP batch holds ONE identity matrix there (prox_pass == 2): lp != 0 says H = 0.
// Rinv, scaling, L, vecs and Mblk are NOT read.
//
// Mapping: one wavefront per problem, n <= 64: lane i owns element i of every n-vector (registers), dot products are butterflies
// over the wavefront, and LDS holds the k reflectors with R above them (k columns of stride n | 1) and, behind them, Hr (n - k
// columns of stride (n - k) | 1: walking a row of it is conflict-free as well) -- n (n | 1) doubles together -- plus three n-vectors:
// 34.8 KB at n = 64, four workgroups per CU.  All arithmetic is fp64.
#pragma once
#include "batch_dev.hip.h"

namespace daqp_amd {

struct NullspaceArgs {
    const double *grad_x;           // [N][n]
    double *dz, *dbupper, *dblower; // [N][n], [N][m], [N][m]
    int *status;                    // [N]
    int lp;                         // the batch is an LP batch: b.H is the setup's identity, H = 0
    int only_prox;                  // 1: only the problems with n_prox > 0 (the others were written by k_backward and stay untouched)
    const double *grad_lam;         // [N][m]: DUAL kernel only (read on W); grad_x may be null there (= 0)
};

__host__ __device__ inline size_t nullspace_lds_bytes(int n) { return ((size_t)n * (n | 1) + 3 * (size_t)n) * sizeof(double); }

__device__ __forceinline__ double ns_wsum(double v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double ns_wmax(double v)
{
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// x <- (I - beta v v') x, v = reflector c (zero above c, one at c): element `lane` of x in every lane, zero in the lanes >= n
__device__ __forceinline__ double ns_reflect(double x, const double *V, const double *beta, int c, int ldn, int lane, int n)
{
    const double v = (lane >= c && lane < n) ? V[(size_t)c * ldn + lane] : 0.0;
    const double d = ns_wsum(v * x);
    return x - (beta[c] * d) * v;
}

// t = H x (H symmetric, n x n row-major in HBM; lp: H = 0): element `lane` of both in every lane
__device__ __forceinline__ double ns_hmul(const double *H, double x, int lane, int n, int lp)
{
    double t = 0.0;
    if (!lp) {
        for (int l = 0; l < n; ++l) {
            const double xl = __shfl(x, l, 64);
            if (lane < n) t += H[(size_t)l * n + lane] * xl;
        }
    }
    return t;
}

// (a template only so that backward_kernel.hip holds the one instantiation: T is the wavefront, 64)
template <int T, bool DUAL = false>
__global__ __launch_bounds__(T) void k_backward_nullspace(BatchDev b, NullspaceArgs a)
{
    static_assert(T == 64, "one wavefront per problem");
    extern __shared__ double lds_ns[];
    const int lane = threadIdx.x, n = b.n, m = b.m, ms = b.ms, cap = b.cap, mA = b.mA;
    const int q = blockIdx.x;
    if (q >= b.N || n > 64) return;
    const QState *qs = b.qs + q;
    if (a.only_prox && !(qs->n_prox > 0)) return;      // (block-uniform)
    const int ldn = n | 1;
    double *V = lds_ns, *beta = V + (size_t)n * ldn, *rd = beta + n, *rn = rd + n;
    double *dzq = a.dz + (size_t)q * n, *dbu = a.dbupper + (size_t)q * m, *dbl = a.dblower + (size_t)q * m;
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
    for (int r = lane; r < m; r += 64) { dbu[r] = 0.0; dbl[r] = 0.0; }
    const size_t qF = qf(b, q);
    const double *H = b.H + qF * (size_t)n * n;
    const double *Aq = b.A + (b.shared ? qF : (size_t)q) * mA * n;
    const int nz = n - k, ldz = nz | 1;
    double *Hr = V + (size_t)k * ldn;      // element (r, c), r >= c, at Hr[c * ldz + r]
    const double g = (st == 0 && lane < n && !(DUAL && !a.grad_x)) ? a.grad_x[(size_t)q * n + lane] : 0.0;

    // ---- 1, 2: the rows of C_W, unit length, and the QR of C_W' one column at a time
    for (int c = 0; st == 0 && c < k; ++c) {
        const int id = b.WS[(size_t)q * cap + c];
        if (id < 0 || id >= m) { st = DAQP_BACKWARD_SINGULAR; break; }
        double x = 0.0;
        if (lane < n) x = (id < ms) ? (lane == id ? 1.0 : 0.0) : Aq[(size_t)(id - ms) * n + lane];
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

    // ---- 4: dz = Z Hr^-1 Z'g, then R dnu~ = Q1'(g - H dz)
    double dz = 0.0;
    if constexpr (DUAL) {
        if (st == 0) {
            // y = R^-T (g_lamW / s), lane i owns entry i (R sits above the reflectors: R(c, i) at V[i * ldn + c])
            double w = 0.0;
            if (lane < k) w = a.grad_lam[(size_t)q * m + b.WS[(size_t)q * cap + lane]] / rn[lane];
            for (int c = 0; c < k; ++c) {
                const double yc = __shfl(w, c, 64) / rd[c];
                if (lane == c) w = yc;
                else if (lane > c && lane < k) w -= V[(size_t)lane * ldn + c] * yc;
            }
            if (nz > 0) {
                // t = g - H Q [y; 0], then z = Hr^-1 (Q't)[k:]
                double p = w;
                for (int c = k - 1; c >= 0; --c) p = ns_reflect(p, V, beta, c, ldn, lane, n);
                double t = g - ns_hmul(H, p, lane, n, 0);
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
            dz = w;      // dz = Q [y; z]
            for (int c = k - 1; c >= 0; --c) dz = ns_reflect(dz, V, beta, c, ldn, lane, n);
        }
    } else if (st == 0 && nz > 0) {
        double y = g;
        for (int c = 0; c < k; ++c) y = ns_reflect(y, V, beta, c, ldn, lane, n);
        // lane r < nz takes entry k + r of Q'g
        double rhs = __shfl(y, (lane + k) & 63, 64);
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
        // back to entry k + r of an n-vector whose first k entries are zero, then dz = Q [0; y2]
        dz = __shfl(rhs, (lane - k) & 63, 64);
        if (lane < k || lane >= n) dz = 0.0;
        for (int c = k - 1; c >= 0; --c) dz = ns_reflect(dz, V, beta, c, ldn, lane, n);
    }
    if (st == 0 && k > 0) {
        double r = g - ns_hmul(H, dz, lane, n, a.lp);
        for (int c = 0; c < k; ++c) r = ns_reflect(r, V, beta, c, ldn, lane, n);
        for (int c = k - 1; c >= 0; --c) {      // R dnu~ = r(0 : k), lane i owns row i
            const double dc = __shfl(r, c, 64) / rd[c];
            if (lane == c) r = dc;
            else if (lane < c) r -= V[(size_t)c * ldn + lane] * dc;
        }
        if (lane < k) {
            const int id = b.WS[(size_t)q * cap + lane];
            const int sg = b.sense[(size_t)q * m + id];
            ((sg & DAQP_LOWER) ? dbl : dbu)[id] = r / rn[lane];
        }
    }
    if (lane < n) dzq[lane] = st == 0 ? dz : 0.0;
    if (lane == 0) a.status[q] = st;
}

} // namespace daqp_amd
