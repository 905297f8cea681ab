// minrep.hip.h -- redundancy removal (daqp_minrep, reference api.c:531-558 / utils.c:808-835) as a batch of LDPs, and the
// reset of a kept workspace (daqp.c:142-146, auxiliary.c:482-497).
//
// P polyhedra {x : A x <= b} of one shape; row i of polyhedron p is redundant iff the face {A_i x = b_i} of p is empty, which is
// one LDP on M = A with row i pinned as an equality (sense ACTIVE|IMMUTABLE) and an INFEASIBLE verdict.  The P * m tests are
// independent: problem q = p * m + i of a batch of N = P * m, all m problems of a polyhedron reading ONE image of M
// (BatchDev::shared = m, see qf()).  The solves are the library's ordinary solve kernels; what is here is what comes before and
// after them:
//   k_minrep_setup   a workgroup per polyhedron: rows of A normalised to unit length (as the QP setup does: the fp32 screen of the
//                    image kernels certifies its margin for rows of norm <= 1 only), the blocked fp64 image, its fp32 copy where
//                    the workgroup kernel wants one, the rows' factors 1 / |A_i| (rowscale), the structural bits of vanishing rows,
//                    and the identity-factor state of the LP path (R^-1 = I, RinvD = 1).  BatchDev::scaling is 1 for every row: the
//                    solve kernels compare a slack with primal_tol * scaling (auxiliary.c:110,136: the QP path's way of holding
//                    the RAW slack to primal_tol), and here the normalised rows ARE the problem -- primal_tol is held against the
//                    slack in units of the row's length, whatever scale the caller's rows have (with scaling = 1 / |A_i| a row of
//                    length 1e-2 was let through with a normalised slack of -1e-4, and a redundant row that clears its bound by
//                    less was kept)
//   k_minrep_init    a wave per test: d = b * rowscale, dlower = -1e30, v = 0, the sense with the pinned row, a fresh record
//   k_minrep_verdict exit flags -> is_redundant (INFEASIBLE: 1, a vanishing row: -1, anything else: 0), other flags than OPTIMAL /
//                    INFEASIBLE counted
//   k_reset          daqp_deactivate_constraints and / or reset_daqp_workspace for every problem of a batch
#pragma once
#include "batch_dev.hip.h"

namespace daqp_amd {

constexpr int kResetDeactivate = 1, kResetWorkspace = 2;

__global__ __launch_bounds__(256) void k_minrep_setup(BatchDev b, const double *A, int *structural, double *rowscale)
{
    const int p = blockIdx.x, tid = threadIdx.x;
    const int n = b.n, m = b.m, ms = b.ms, mA = b.mA;
    double2 *Mq = reinterpret_cast<double2 *>(b.Mblk + (size_t)p * b.nblk * b.npair * 128);
    float *M32 = b.M32 ? b.M32 + (size_t)p * b.nblk * b.nquad * 256 : nullptr;
    double *sc = b.scaling + (size_t)p * m, *rs = rowscale + (size_t)p * m;
    int *str = structural + (size_t)p * m;
    const double *Ap = A + (size_t)p * mA * n;
    // R^-1 = I, packed upper triangle (the back-transformation of the solve kernels reads it)
    double *Rq = b.Rinv + (size_t)p * b.rtri;
    for (int e = tid; e < b.rtri; e += 256) Rq[e] = 0.0;
    __syncthreads();
    for (int i = tid; i < n; i += 256) Rq[roff(i, n) + i] = 1.0;
    // a thread per row: simple bounds are exact unit vectors, general rows are normalised (sum of squares in column order)
    for (int r = tid; r < m; r += 256) {
        double2 *dst = Mq + ((size_t)(r >> 6) * b.npair) * 64 + (r & 63);
        float *d32 = M32 ? M32 + (((size_t)(r >> 6) * b.nquad) * 64 + (r & 63)) * 4 : nullptr;
        double scal = 1.0;
        int sbits = 0;
        const double *row = r >= ms ? Ap + (size_t)(r - ms) * n : nullptr;
        if (row) {
            double s = 0;
            for (int k = 0; k < n; ++k) s += row[k] * row[k];
            if (s < b.st.zero_tol) sbits = DAQP_IMMUTABLE;      // utils.c:586-613: a vanishing row takes no part
            else scal = 1 / sqrt(s);
        }
        for (int t = 0; t < b.npair; ++t) {
            double2 w;
            const int k0 = 2 * t, k1 = 2 * t + 1;
            if (row) { w.x = row[k0] * scal; w.y = k1 < n ? row[k1] * scal : 0.0; }
            else { w.x = k0 == r ? 1.0 : 0.0; w.y = k1 == r ? 1.0 : 0.0; }
            dst[(size_t)t * 64] = w;
            if (d32) { float *q4 = d32 + (size_t)(t >> 1) * 256 + 2 * (t & 1); q4[0] = (float)w.x; q4[1] = (float)w.y; }
        }
        if (d32 && (b.npair & 1)) { float *q4 = d32 + (size_t)(b.npair >> 1) * 256 + 2; q4[0] = 0.0f; q4[1] = 0.0f; }
        sc[r] = 1.0;
        rs[r] = scal;
        str[r] = sbits;
    }
}

__global__ __launch_bounds__(64) void k_minrep_init(BatchDev b, const double *rhs, const int *structural, const double *rowscale)
{
    const int q = blockIdx.x, lane = threadIdx.x, m = b.m, n = b.n;
    const int p = q / m, i = q - p * m;
    const double *sc = rowscale + (size_t)p * m, *bp = rhs + (size_t)p * m;
    const int *str = structural + (size_t)p * m;
    const int pinned = !(str[i] & DAQP_IMMUTABLE);
    for (int r = lane; r < m; r += 64) {
        b.dupper[(size_t)q * m + r] = bp[r] * sc[r];
        b.dlower[(size_t)q * m + r] = -DAQP_INF;
        int s = str[r];
        if (r == i && pinned) s = DAQP_ACTIVE | DAQP_IMMUTABLE;
        b.sense[(size_t)q * m + r] = s;
    }
    for (int k = lane; k < n; k += 64) b.v[(size_t)q * n + k] = 0.0;
    for (int k = lane; k < 5 * b.cap; k += 64) b.vecs[(size_t)q * 5 * b.cap + k] = 0.0;
    for (int k = lane; k < b.cap; k += 64) b.WS[(size_t)q * b.cap + k] = -1;
    if (lane == 0) {
        QState *qs = b.qs + q;
        qs->n_active = 0; qs->reuse_ind = 0; qs->sing_ind = kEmpty; qs->iterations = 0;
        qs->lam_swapped = 0; qs->setup_flag = 1; qs->need_activate = pinned; qs->pad_ = 0;
        qs->exitflag = 1; qs->fval = 0; qs->soft_slack = 0; qs->diag_h = 1; qs->n_prox = 0;
        qs->upd_flag = 0;
    }
}

__global__ __launch_bounds__(256) void k_minrep_verdict(int N, int m, const int *exitflag, const int *structural, int *is_redundant, int *other)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= N) return;
    if (structural[q] & DAQP_IMMUTABLE) { is_redundant[q] = -1; return; }      // (structural is [P][m]: the same index as the test's)
    const int f = exitflag[q];
    is_redundant[q] = f == DAQP_EXIT_INFEASIBLE ? 1 : 0;
    if (f != DAQP_EXIT_INFEASIBLE && f != DAQP_EXIT_OPTIMAL) atomicAdd(other, 1);
    (void)m;
}

// what & kResetDeactivate: the ACTIVE bit of every working-set row that is not IMMUTABLE goes, and the working set with it; the stored
// factor and multipliers count as empty (the next solve starts where a solve straight after the setup starts).
// what & kResetWorkspace: sing_ind = EMPTY, reuse_ind = 0, n_active = 0, iterations = 0.
__global__ __launch_bounds__(64) void k_reset(BatchDev b, int what)
{
    const int q = blockIdx.x, lane = threadIdx.x, m = b.m, cap = b.cap;
    QState *qs = b.qs + q;
    if (qs->setup_flag < 0) return;
    const int na = qs->n_active;
    if (what & kResetDeactivate) {
        for (int k = lane; k < na && k < cap; k += 64) {
            const int id = b.WS[(size_t)q * cap + k];
            if (id >= 0 && id < m) {
                const int s = b.sense[(size_t)q * m + id];
                if (!(s & DAQP_IMMUTABLE)) b.sense[(size_t)q * m + id] = s & ~DAQP_ACTIVE;
            }
        }
    }
    for (int k = lane; k < 5 * cap; k += 64) b.vecs[(size_t)q * 5 * cap + k] = 0.0;
    for (int k = lane; k < cap; k += 64) b.WS[(size_t)q * cap + k] = -1;
    if (lane == 0) {
        qs->n_active = 0; qs->lam_swapped = 0; qs->fval = 0; qs->soft_slack = 0;
        if (what & kResetWorkspace) { qs->sing_ind = kEmpty; qs->reuse_ind = 0; qs->iterations = 0; }
    }
}

} // namespace daqp_amd
