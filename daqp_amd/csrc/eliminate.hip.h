// eliminate.hip.h -- equality rows of a batch eliminated on the device: reduce (k_eliminate, k_eliminate_update), solve the reduced
// batch with the ordinary solve path, expand (k_expand).  Additive: nothing here runs inside a setup or a solve.
//
// Per problem, with C = [first ms rows of I; A] (m rows), E the neq equality rows (one row set for the whole batch), e = bupper_E and
// I the m - neq kept rows in their original order:
//
//     1. QR        the rows of E scaled to unit length (norms kept), Householder QR of E' (n x neq) without pivoting, left-looking:
//                  E' = Q [R; 0], Q = [Q1 Z].  R_jj^2 < zero_tol: the rows are dependent, DAQP_EXIT_OVERDETERMINED_INITIAL, every
//                  reduced array of that problem is zero (the rule and the reflector layout of nullspace.hip.h: column c holds R
//                  above the diagonal, one on it, the reflector below; R_cc, beta_c and the row norm in three vectors).
//     2. x0        R'w = e / |row|, x0 = Q [w; 0]: the minimum-norm solution of E x = e.  bupper != blower on a row of E: the problem
//                  is no equality problem, DAQP_EXIT_UNSUPPORTED, x0 = f_r = c0 = 0 and its reduced bounds are zero.
//     3. f_r, c0   g = H x0 + f, f_r = (Q'g)(neq:), c0 = x0'(1/2 H x0 + f); an LP (H == NULL) has g = f
//     4. rows      every kept row c_k is read once, one element per lane: bupper_r = bupper_k - c_k x0 (an open bound, |b| >= DAQP_INF,
//                  stays as it is), blower_r likewise, A_r row = (Q'c_k')(neq:) -- the reflectors applied in registers
//     5. H_r       M = H, then M <- H_c M H_c for c = 0 .. neq-1 as symmetric rank-two updates of the trailing block
//                  (p = M v, w = beta p - (beta^2 v'p / 2) v, M -= v w' + w v'); H_r is the last nr x nr block, its lower triangle
//                  mirrored.  Z is never formed.
//
// k_eliminate_update runs 2 - 4 (without A_r) on the kept Q, R through the same device functions, wave for wave in the same order:
// its outputs are the bits a fresh k_eliminate writes.
//
// Expansion of a reduced result (y, lam_r, fval_r):  x = x0 + Q [0; y],  lam_I = lam_r,  R lam~ = -(Q'(H x + f + C_I'lam_I))(0:neq),
// lam_E = lam~ / |row|,  fval = fval_r + c0.
//
// Mapping.  A vector of n entries lives in the registers of ONE wavefront, NV = ceil(n / 64) entries per lane (entry lane + 64 e);
// dot products are butterflies over the wavefront.  n <= 64: one wavefront per problem, M and the reflectors in LDS
// ((n^2 + neq (n | 1) + 3 neq + 4 n) doubles: 69 088 B = 69.1 KB at n = 64, neq = 63 -- two workgroups per CU, LDS-bound).  64 < n <= 511: one
// workgroup of four wavefronts per problem, persistent; M lives in the handle's scratch (n^2 doubles per workgroup, L2-resident),
// the reflectors in the handle's V, the current reflector and the work vectors in LDS.  The four wavefronts run the QR side by side
// on identical values (wave 0 stores), share the kept rows among them and run step 5 together, one column of M per thread.
// ONLY k_eliminate has the workgroup tier: k_eliminate_update, k_expand and k_elim_basis are one wavefront per problem at every n (up to
// eight entries per lane, H x as one serial sweep of the wavefront over n columns) and read the kept factor from global memory.
// All arithmetic is fp64, no contraction.
#pragma once
#include "nullspace.hip.h"

namespace daqp_amd {

struct ElimDev {
    int N, n, m, ms, neq, nr, mr, ldn, lp;
    double zero_tol;
    // the caller's problem (device pointers: borrowed, or the handle's copies of host arrays); H null for an LP, sense may be null
    const double *H, *f, *A, *bu, *bl;
    const int *sense;
    const int *eq_rows, *kept;       // [neq], [mr]: original row indices, ascending
    // kept factor
    double *V;                       // [N][neq][ldn]
    double *beta, *rd, *rn;          // [N][neq]
    double *x0, *c0;                 // [N][n], [N]
    int *flags;                      // [N]: 1, DAQP_EXIT_OVERDETERMINED_INITIAL, DAQP_EXIT_UNSUPPORTED
    // reduced problem (nr, mr, 0)
    double *Hr, *fr, *Ar, *bur, *blr;
    int *senser;
    double *scratch;                 // [grid][n * n], workgroup tier only
};

struct ExpandArgs {
    const double *y, *lamr, *fvalr, *softr;      // [N][nr], [N][mr], [N], [N]
    const int *flagr, *iterr;
    double *x, *lam, *fval, *soft;               // [N][n], [N][m], [N], [N]; any may be null
    int *exitflag, *iter;
};

__host__ __device__ inline int elim_nv(int n) { return n <= 64 ? 1 : (n <= 128 ? 2 : (n <= 256 ? 4 : 8)); }
__host__ __device__ inline size_t elim_lds_bytes(int n, int neq, bool wave)
{
    return (3 * (size_t)neq + 4 * (size_t)n + (wave ? (size_t)n * n + (size_t)neq * (n | 1) : 0)) * sizeof(double);
}

template <int NV>
__device__ __forceinline__ double el_dot(const double (&a)[NV], const double (&b)[NV])
{
    double s = 0.0;
#pragma unroll
    for (int e = 0; e < NV; ++e) s += a[e] * b[e];
    return ns_wsum(s);
}

// entry c of a vector, in every lane
template <int NV>
__device__ __forceinline__ double el_bcast(const double (&x)[NV], int c)
{
    double v = x[0];
#pragma unroll
    for (int e = 1; e < NV; ++e)
        if ((c >> 6) == e) v = x[e];
    return __shfl(v, c & 63, 64);
}

// x <- (I - beta_c v v') x, v = reflector c
template <int NV>
__device__ __forceinline__ void el_reflect(double (&x)[NV], const double *V, const double *beta, int c, int ldn, int lane, int n)
{
    if constexpr (NV == 1) {
        x[0] = ns_reflect(x[0], V, beta, c, ldn, lane, n);
    } else {
        double v[NV], s = 0.0;
#pragma unroll
        for (int e = 0; e < NV; ++e) {
            const int i = lane + 64 * e;
            v[e] = (i >= c && i < n) ? V[(size_t)c * ldn + i] : 0.0;
            s += v[e] * x[e];
        }
        const double bd = beta[c] * ns_wsum(s);
#pragma unroll
        for (int e = 0; e < NV; ++e) x[e] -= bd * v[e];
    }
}

// row r of C = [first ms rows of I; A] of problem q, zero beyond n
template <int NV>
__device__ __forceinline__ void el_row(double (&x)[NV], const ElimDev &d, int q, int r, int lane)
{
    const double *Aq = d.A + (size_t)q * (d.m - d.ms) * d.n;
#pragma unroll
    for (int e = 0; e < NV; ++e) {
        const int i = lane + 64 * e;
        x[e] = 0.0;
        if (i < d.n) x[e] = r < d.ms ? (i == r ? 1.0 : 0.0) : Aq[(size_t)(r - d.ms) * d.n + i];
    }
}

// t = H x for the x held in xs (LDS, n entries); H symmetric: lane i walks column i
template <int NV>
__device__ __forceinline__ void el_hmul(double (&t)[NV], const double *Hq, const double *xs, int lane, int n)
{
#pragma unroll
    for (int e = 0; e < NV; ++e) t[e] = 0.0;
    for (int l = 0; l < n; ++l) {
        const double xl = xs[l];
#pragma unroll
        for (int e = 0; e < NV; ++e) {
            const int i = lane + 64 * e;
            if (i < n) t[e] += Hq[(size_t)l * n + i] * xl;
        }
    }
}

// 1: the QR of the unit equality rows.  Every wavefront of the block runs it on the same values; `store`: this one writes.
// V, beta, rd, rn: LDS or global, read back by the block after the barrier that ends each column.  false: dependent rows.
template <int NV>
__device__ bool el_qr(const ElimDev &d, int q, double *V, double *beta, double *rd, double *rn, bool store, int lane)
{
    const int n = d.n, ldn = d.ldn;
    for (int c = 0; c < d.neq; ++c) {
        double x[NV];
        el_row<NV>(x, d, q, d.eq_rows[c], lane);
        const double len2 = el_dot<NV>(x, x);
        if (!(len2 > 0.0)) return false;
        const double len = sqrt(len2);
#pragma unroll
        for (int e = 0; e < NV; ++e) x[e] /= len;
        for (int j = 0; j < c; ++j) el_reflect<NV>(x, V, beta, j, ldn, lane, n);
        double s = 0.0;
#pragma unroll
        for (int e = 0; e < NV; ++e) s += (lane + 64 * e >= c) ? x[e] * x[e] : 0.0;
        const double sigma = ns_wsum(s);      // R_cc^2
        if (!(sigma >= d.zero_tol)) return false;
        const double alpha = el_bcast<NV>(x, c);
        const double rcc = alpha >= 0.0 ? -sqrt(sigma) : sqrt(sigma);
        const double u0 = alpha - rcc;      // (|u0| >= |R_cc| > 0)
        if (store) {
#pragma unroll
            for (int e = 0; e < NV; ++e) {
                const int i = lane + 64 * e;
                if (i < n) V[(size_t)c * ldn + i] = i < c ? x[e] : (i == c ? 1.0 : x[e] / u0);
            }
            if (lane == 0) { beta[c] = -u0 / rcc; rd[c] = rcc; rn[c] = len; }
        }
        __syncthreads();
    }
    return true;
}

// every equality row has bupper == blower (wave-uniform)
__device__ __forceinline__ bool el_eq_ok(const ElimDev &d, int q, int lane)
{
    double bad = 0.0;
    for (int c = lane; c < d.neq; c += 64) {
        const size_t k = (size_t)q * d.m + d.eq_rows[c];
        if (d.bu[k] != d.bl[k]) bad = 1.0;
    }
    return !(ns_wmax(bad) > 0.0);
}

// 2: x0 = Q [R^-T (e / |row|); 0]
template <int NV>
__device__ __forceinline__ void el_x0(double (&w)[NV], const ElimDev &d, int q, const double *V, const double *beta, const double *rd,
                                      const double *rn, int lane)
{
    const int n = d.n, ldn = d.ldn;
#pragma unroll
    for (int e = 0; e < NV; ++e) w[e] = 0.0;
    for (int c = 0; c < d.neq; ++c) {      // R'w = e~, row by row: R(j, c), j < c, is V[c][j]
        double s = 0.0;
#pragma unroll
        for (int e = 0; e < NV; ++e) {
            const int i = lane + 64 * e;
            if (i < c) s += V[(size_t)c * ldn + i] * w[e];
        }
        const double wc = (d.bu[(size_t)q * d.m + d.eq_rows[c]] / rn[c] - ns_wsum(s)) / rd[c];
#pragma unroll
        for (int e = 0; e < NV; ++e)
            if (lane + 64 * e == c) w[e] = wc;
    }
    for (int c = d.neq - 1; c >= 0; --c) el_reflect<NV>(w, V, beta, c, ldn, lane, n);
}

__device__ __forceinline__ double el_shift(double b, double cx) { return (b >= DAQP_INF || b <= -DAQP_INF) ? b : b - cx; }

// 2 - 4 for problem q on a kept factor: x0, f_r, c0, the reduced bounds and, WITH_A, A_r and sense_r.  The block's W wavefronts share the
// kept rows; wave 0 writes everything else.  flag < 0: the outputs that depend on f and the bounds are zero.  xs: n doubles of LDS.
template <int NV, bool WITH_A>
__device__ void el_rhs(const ElimDev &d, int q, const double *V, const double *beta, const double *rd, const double *rn, double *xs,
                       int flag, int wave, int W, int lane)
{
    const int n = d.n, neq = d.neq, nr = d.nr, mr = d.mr, ldn = d.ldn;
    double x0[NV];
    if (flag > 0) el_x0<NV>(x0, d, q, V, beta, rd, rn, lane);
    else {
#pragma unroll
        for (int e = 0; e < NV; ++e) x0[e] = 0.0;
    }
    if (wave == 0) {
#pragma unroll
        for (int e = 0; e < NV; ++e) {
            const int i = lane + 64 * e;
            if (i < n) { xs[i] = x0[e]; d.x0[(size_t)q * n + i] = x0[e]; }
        }
    }
    __syncthreads();
    if (wave == 0) {
        double t[NV], g[NV], s = 0.0;
        if (d.lp) {
#pragma unroll
            for (int e = 0; e < NV; ++e) t[e] = 0.0;
        } else el_hmul<NV>(t, d.H + (size_t)q * n * n, xs, lane, n);
#pragma unroll
        for (int e = 0; e < NV; ++e) {
            const int i = lane + 64 * e;
            const double fi = (i < n && flag > 0) ? d.f[(size_t)q * n + i] : 0.0;
            s += x0[e] * (0.5 * t[e] + fi);
            g[e] = t[e] + fi;
        }
        const double c0 = ns_wsum(s);
        for (int c = 0; c < neq; ++c) el_reflect<NV>(g, V, beta, c, ldn, lane, n);
#pragma unroll
        for (int e = 0; e < NV; ++e) {
            const int i = lane + 64 * e;
            if (i >= neq && i < n) d.fr[(size_t)q * nr + (i - neq)] = g[e];
        }
        if (lane == 0) d.c0[q] = c0;
    }
    for (int j = wave; j < mr; j += W) {
        const int r = d.kept[j];
        double crow[NV];
        el_row<NV>(crow, d, q, r, lane);
        double bu = 0.0, bl = 0.0;
        if (flag > 0) {
            const double cx = el_dot<NV>(crow, x0);
            bu = el_shift(d.bu[(size_t)q * d.m + r], cx);
            bl = el_shift(d.bl[(size_t)q * d.m + r], cx);
        }
        if (lane == 0) { d.bur[(size_t)q * mr + j] = bu; d.blr[(size_t)q * mr + j] = bl; }
        if constexpr (WITH_A) {
            for (int c = 0; c < neq; ++c) el_reflect<NV>(crow, V, beta, c, ldn, lane, n);
#pragma unroll
            for (int e = 0; e < NV; ++e) {
                const int i = lane + 64 * e;
                if (i >= neq && i < n) d.Ar[((size_t)q * mr + j) * nr + (i - neq)] = crow[e];
            }
            if (lane == 0) d.senser[(size_t)q * mr + j] = d.sense ? d.sense[(size_t)q * d.m + r] : 0;
        }
    }
}

// NV entries per lane, W wavefronts per block.  W == 1 (n <= 64): one problem per block; W > 1: persistent blocks.
template <int NV, int W>
__global__ __launch_bounds__(64 * W) void k_eliminate(ElimDev d)
{
    static_assert((NV == 1) == (W == 1), "one wavefront for n <= 64, a workgroup beyond");
    extern __shared__ double lds_el[];
    constexpr int T = 64 * W;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = d.n, neq = d.neq, nr = d.nr, mr = d.mr, ldn = d.ldn;
    if (n > 64 * NV || neq < 1 || neq >= n) return;
    double *beta = lds_el, *rd = beta + neq, *rn = rd + neq, *xs = rn + neq, *pv = xs + n, *wv = pv + n, *vv = wv + n;
    for (int q = blockIdx.x; q < d.N; q += gridDim.x) {
        double *Vg = d.V + (size_t)q * neq * ldn;
        double *V = W == 1 ? vv + n + (size_t)n * n : Vg;
        double *M = W == 1 ? vv + n : d.scratch + (size_t)blockIdx.x * n * n;      // element (i, j) at M[j * n + i]: thread i walks column i
        __syncthreads();
        const bool ok = el_qr<NV>(d, q, V, beta, rd, rn, wave == 0, lane);      // (block-uniform)
        if (!ok) {
            for (int i = tid; i < n; i += T) d.x0[(size_t)q * n + i] = 0.0;
            for (int i = tid; i < nr; i += T) d.fr[(size_t)q * nr + i] = 0.0;
            if (!d.lp)      // (an LP batch has no H_r: the buffer is one element)
                for (int i = tid; i < nr * nr; i += T) d.Hr[(size_t)q * nr * nr + i] = 0.0;
            for (int i = tid; i < mr * nr; i += T) d.Ar[(size_t)q * mr * nr + i] = 0.0;
            for (int i = tid; i < mr; i += T) { d.bur[(size_t)q * mr + i] = 0.0; d.blr[(size_t)q * mr + i] = 0.0; d.senser[(size_t)q * mr + i] = 0; }
            if (tid == 0) { d.c0[q] = 0.0; d.flags[q] = DAQP_EXIT_OVERDETERMINED_INITIAL; }
            continue;
        }
        for (int i = tid; i < neq; i += T) {
            d.beta[(size_t)q * neq + i] = beta[i]; d.rd[(size_t)q * neq + i] = rd[i]; d.rn[(size_t)q * neq + i] = rn[i];
        }
        if (W == 1)
            for (int i = tid; i < neq * ldn; i += T)
                if (i % ldn < n) Vg[i] = V[i];
        const int flag = el_eq_ok(d, q, lane) ? 1 : DAQP_EXIT_UNSUPPORTED;
        if (tid == 0) d.flags[q] = flag;
        el_rhs<NV, true>(d, q, V, beta, rd, rn, xs, flag, wave, W, lane);
        if (d.lp) continue;

        // ---- 5: H_r.  M = H, then the reflectors from both sides on the trailing block
        const double *Hq = d.H + (size_t)q * n * n;
        for (int i = tid; i < n; i += T)
            for (int j = 0; j < n; ++j) M[(size_t)j * n + i] = Hq[(size_t)j * n + i];
        for (int c = 0; c < neq; ++c) {
            __syncthreads();
            for (int i = tid; i < n; i += T) vv[i] = i < c ? 0.0 : V[(size_t)c * ldn + i];
            __syncthreads();
            for (int i = c + tid; i < n; i += T) {      // p = M v
                double p = 0.0;
                for (int j = c; j < n; ++j) p += M[(size_t)j * n + i] * vv[j];
                pv[i] = p;
            }
            __syncthreads();
            double s = 0.0;      // v'p, in every wavefront in the same order
            for (int i = lane; i < n; i += 64) s += i >= c ? vv[i] * pv[i] : 0.0;
            const double bc = beta[c], half = 0.5 * bc * bc * ns_wsum(s);
            for (int i = c + tid; i < n; i += T) wv[i] = bc * pv[i] - half * vv[i];
            __syncthreads();
            for (int i = c + tid; i < n; i += T) {      // M -= v w' + w v': the same bits at (i, j) and (j, i)
                const double vi = vv[i], wi = wv[i];
                for (int j = c; j < n; ++j) M[(size_t)j * n + i] -= vi * wv[j] + wi * vv[j];
            }
        }
        __syncthreads();
        for (int i = neq + tid; i < n; i += T)      // one triangle, mirrored
            for (int j = neq; j <= i; ++j) {
                const double h = M[(size_t)j * n + i];
                d.Hr[((size_t)q * nr + (i - neq)) * nr + (j - neq)] = h;
                d.Hr[((size_t)q * nr + (j - neq)) * nr + (i - neq)] = h;
            }
    }
}

// new f and / or bounds on the kept factor: 2 - 4 without A_r.  One wavefront per problem.
template <int NV>
__global__ __launch_bounds__(64) void k_eliminate_update(ElimDev d)
{
    __shared__ double xs[64 * NV];
    const int lane = threadIdx.x, q = blockIdx.x, neq = d.neq;
    if (q >= d.N || d.n > 64 * NV) return;
    if (d.flags[q] == DAQP_EXIT_OVERDETERMINED_INITIAL) return;      // no factor: everything is zero and stays so
    const int flag = el_eq_ok(d, q, lane) ? 1 : DAQP_EXIT_UNSUPPORTED;
    el_rhs<NV, false>(d, q, d.V + (size_t)q * neq * d.ldn, d.beta + (size_t)q * neq, d.rd + (size_t)q * neq, d.rn + (size_t)q * neq, xs,
                      flag, 0, 1, lane);
    if (lane == 0) d.flags[q] = flag;
}

// the expansion of a reduced result.  One wavefront per problem.
template <int NV>
__global__ __launch_bounds__(64) void k_expand(ElimDev d, ExpandArgs a)
{
    __shared__ double xs[64 * NV];
    const int lane = threadIdx.x, q = blockIdx.x, n = d.n, m = d.m, neq = d.neq, nr = d.nr, mr = d.mr, ldn = d.ldn;
    if (q >= d.N || n > 64 * NV) return;
    const int flag = d.flags[q];
    if (lane == 0) {
        if (a.exitflag) a.exitflag[q] = flag < 0 ? flag : a.flagr[q];
        if (a.iter) a.iter[q] = a.iterr ? a.iterr[q] : 0;
        if (a.soft) a.soft[q] = a.softr ? a.softr[q] : 0.0;
        if (a.fval) a.fval[q] = flag < 0 ? 0.0 : (a.fvalr ? a.fvalr[q] : 0.0) + d.c0[q];
    }
    if (flag < 0) {
        if (a.x) for (int i = lane; i < n; i += 64) a.x[(size_t)q * n + i] = 0.0;
        if (a.lam) for (int i = lane; i < m; i += 64) a.lam[(size_t)q * m + i] = 0.0;
        return;
    }
    const double *V = d.V + (size_t)q * neq * ldn, *beta = d.beta + (size_t)q * neq, *rd = d.rd + (size_t)q * neq, *rn = d.rn + (size_t)q * neq;
    // x = x0 + Q [0; y]
    double x[NV];
#pragma unroll
    for (int e = 0; e < NV; ++e) {
        const int i = lane + 64 * e;
        x[e] = (i >= neq && i < n) ? a.y[(size_t)q * nr + (i - neq)] : 0.0;
    }
    for (int c = neq - 1; c >= 0; --c) el_reflect<NV>(x, V, beta, c, ldn, lane, n);
#pragma unroll
    for (int e = 0; e < NV; ++e) {
        const int i = lane + 64 * e;
        if (i < n) {
            x[e] += d.x0[(size_t)q * n + i];
            xs[i] = x[e];
            if (a.x) a.x[(size_t)q * n + i] = x[e];
        }
    }
    if (!a.lam) return;
    __syncthreads();
    for (int j = lane; j < mr; j += 64) a.lam[(size_t)q * m + d.kept[j]] = a.lamr[(size_t)q * mr + j];
    // g = H x + f + C_I' lam_I
    double g[NV];
    if (d.lp) {
#pragma unroll
        for (int e = 0; e < NV; ++e) g[e] = 0.0;
    } else el_hmul<NV>(g, d.H + (size_t)q * n * n, xs, lane, n);
#pragma unroll
    for (int e = 0; e < NV; ++e) {
        const int i = lane + 64 * e;
        if (i < n) g[e] += d.f[(size_t)q * n + i];
    }
    const double *Aq = d.A + (size_t)q * (m - d.ms) * n;
    for (int j = 0; j < mr; ++j) {
        const double l = a.lamr[(size_t)q * mr + j];      // (wave-uniform)
        if (l == 0.0) continue;
        const int r = d.kept[j];
#pragma unroll
        for (int e = 0; e < NV; ++e) {
            const int i = lane + 64 * e;
            if (i < n) g[e] += (r < d.ms ? (i == r ? 1.0 : 0.0) : Aq[(size_t)(r - d.ms) * n + i]) * l;
        }
    }
    // R lam~ = -(Q'g)(0:neq), column by column; lam_E = lam~ / |row|
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
        if (i < neq) a.lam[(size_t)q * m + d.eq_rows[i]] = -g[e] / rn[i];
    }
}

// Z = the last nr columns of Q, n x nr row-major per problem (zeros where there is no factor).  One wavefront per problem.
template <int NV>
__global__ __launch_bounds__(64) void k_elim_basis(ElimDev d, double *Z)
{
    const int lane = threadIdx.x, q = blockIdx.x, n = d.n, neq = d.neq, nr = d.nr, ldn = d.ldn;
    if (q >= d.N || n > 64 * NV) return;
    const bool none = d.flags[q] == DAQP_EXIT_OVERDETERMINED_INITIAL;
    const double *V = d.V + (size_t)q * neq * ldn, *beta = d.beta + (size_t)q * neq;
    for (int j = 0; j < nr; ++j) {
        double z[NV];
#pragma unroll
        for (int e = 0; e < NV; ++e) z[e] = (!none && lane + 64 * e == neq + j) ? 1.0 : 0.0;
        if (!none)
            for (int c = neq - 1; c >= 0; --c) el_reflect<NV>(z, V, beta, c, ldn, lane, n);
#pragma unroll
        for (int e = 0; e < NV; ++e) {
            const int i = lane + 64 * e;
            if (i < n) Z[((size_t)q * n + i) * nr + j] = z[e];
        }
    }
}

} // namespace daqp_amd
