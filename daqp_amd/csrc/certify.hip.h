// certify.hip.h -- the KKT residuals and Farkas measures of a batch of (x, lam) pairs, in twice the working precision.
//
//     min 1/2 x'Hx + f'x   s.t.   blower <= C x <= bupper,   C = [I_ms ; A],   H x + f + C'lam = 0,  lam_k > 0 on an upper bound
//
// Stateless: the kernel reads the caller's H, f, A, bupper, blower, sense, x and lam and nothing else -- no factor, no working set, no
// exit flag -- so it certifies the answer of any solver.  Per problem (definitions: include/daqp_amd.h, daqp_certify_batch; they restate
// tests/kkt_reference.py, certificate(normalised=False), every q_k = 1):
//
//     stationarity        max_j |(Hx + f + C'lam)_j|
//     stationarity_scale  max(1, max_j |(Hx)_j|, max_j |f_j|, max_j |(C'|lam|)_j|)      (C'|lam|: C with its signs, as the reference has it)
//     primal, primal_row  largest max(c_k x - bupper_k, blower_k - c_k x, 0) over the held rows, and where (-1: nowhere above 0)
//     complementarity     largest distance of a row with a multiplier from the bound its sign names; of an equality from its bound
//     wrong_sign          rows with a multiplier whose nearer bound is not the one its sign names
//     objective           1/2 x'Hx + f'x
//     ray_residual        max_j |(C'lam)_j|,   ray_scale  max_j |(C'|lam|)_j|,   ray_support  sum_k lam_k * (bupper_k | blower_k by sign)
//
// A ray (C'lam = 0) with negative support proves {blower <= Cx <= bupper} empty: 0 = lam'Cx <= ray_support for every feasible x.  SOFT
// rows enter the three ray measures as they are: a soft row may be violated, so a ray with weight on one PROVES NOTHING.
//
// ---- arithmetic.  Every inner product and sum is carried as an unevaluated pair (hi, lo): products split error-free with one fma
// (TwoProduct), hi accumulated error-free (TwoSum: Knuth's six operations, no ordering assumed), the two error terms added to lo in
// plain fp64 -- the compensated dot product of Ogita, Rump and Oishi (Dot2), whose result is hi + lo rounded ONCE at the end.  Lanes and
// waves are combined on pairs in the same way (TwoSum on the hi parts, the los added), in a fixed order: the bits do not depend on the
// launch.  For a quantity that is a sum of K terms (products of two inputs) with S = sum |terms|:
//
//     |computed - exact| <= 2^-52 |exact| + (K + 2)^2 2^-104 S
//
// Derivation (u = 2^-53): the exact sum equals hi_final + sum of the <= K product errors r_i (|r_i| <= u |term_i|) and the <= K - 1
// TwoSum errors q_i (sum |q_i| <= gamma_(K-1) S), all of which are added into lo by at most 2K - 1 floating additions in some
// tree: |lo - (sum r + sum q)| <= gamma_(2K-1) (K u S)(1 + ..) < 2 K^2 u^2 S (1 + ..) < (K + 2)^2 2^-105 S for K u << 1; the final
// rounding of hi + lo adds u |result|.  (Ogita-Rump-Oishi, SIAM J. Sci. Comput. 26 (2005), Prop. 5.5, give u |exact| + gamma_K^2 S for
// the sequential order.)  x'Hx multiplies the pair (Hx)_i by x_i (TwoProduct on hi, one rounded product on lo: relative 2u on a term
// that is itself <= 2u S): second order as well.  A max over rows or columns inherits the bound of its rows; which bound is nearer is
// decided on the pair 2 c_k x - (bupper_k + blower_k), which row is the largest on the rounded values.  NaN is never dropped by a max: a NaN in x makes every output
// that depends on x NaN.  Non-finite inputs give non-finite outputs.  The build has -ffp-contract=off: the only fused operations are the
// explicit fma of TwoProduct.
//
// ---- mapping.  A (row-major, n contiguous) and H are read from HBM once, coalesced, lanes across columns.
//   k_certify_wave  n <= 64: one wavefront per problem, four problems per 256-thread block.  W = the power of two >= n; the wave holds
//                   64 / W rows at a time (lane = row slot * W + column), so a row of 12 doubles does not leave 52 lanes idle.  c_k x and
//                   (Hx)_i: one pair butterfly over the W lanes of a slot per row.  C'lam, C'|lam|, Hx + f: per-lane pairs, combined
//                   over the slots once at the end.  No LDS.
//   k_certify_wg    65 <= n <= 511: one workgroup of four waves per problem; wave w takes rows w, w + 4, ...; lane l holds columns
//                   l, l + 64, ... (up to eight, in registers: every loop over them is unrolled and indexed by constants).  The
//                   per-wave column pairs meet in LDS (3 quantities x 4 waves x n rounded up to 64 x 16 bytes: 48 KiB at n = 200),
//                   are added in wave order, and the per-wave row results follow through 4 x 16 doubles of LDS.
// Simple-bound rows (k < ms) touch no matrix: c_k x = x_k.  H == NULL (an LP) skips every H term.  shared: one H and one A for all.
#pragma once
#include <hip/hip_runtime.h>

namespace daqp_amd {

struct CertifyArgs {
    int N, n, m, ms, shared;
    const double *H, *f, *A, *bupper, *blower;   // H may be null (LP); [N] or one (shared) matrices, per-problem vectors
    const int *sense;                             // may be null: all zero
    const double *x, *lam;                        // [N][n], [N][m]
    double *stationarity, *stationarity_scale, *primal, *complementarity, *objective, *ray_residual, *ray_scale, *ray_support;   // [N] each, any may be null
    int *wrong_sign, *primal_row;                 // [N] each, any may be null
};

constexpr int kCertWaves = 4;      // waves of a k_certify_wg block; problems of a k_certify_wave block
constexpr int kCertMaxNC = 8;      // columns per lane of k_certify_wg: n <= 511
constexpr int kCertSenseImmutable = 4, kCertSenseSoft = 8;
__host__ __device__ inline size_t certify_wg_lds_bytes(int n)
{
    return ((size_t)3 * kCertWaves * ((n + 63) / 64 * 64) * 2 + (size_t)kCertWaves * 16) * sizeof(double);
}

struct dd { double hi, lo; };

__device__ __forceinline__ dd dd_two_sum(double a, double b)
{
    const double s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}
__device__ __forceinline__ dd dd_two_prod(double a, double b)
{
    const double p = a * b;
    return {p, fma(a, b, -p)};
}
// acc += t (both pairs): hi error-free, the errors into lo
__device__ __forceinline__ void dd_acc(dd &acc, dd t)
{
    const dd s = dd_two_sum(acc.hi, t.hi);
    acc.hi = s.hi;
    acc.lo += s.lo + t.lo;
}
__device__ __forceinline__ void dd_acc(dd &acc, double t)
{
    const dd s = dd_two_sum(acc.hi, t);
    acc.hi = s.hi;
    acc.lo += s.lo;
}
__device__ __forceinline__ double dd_round(dd a) { return a.hi + a.lo; }
// t + b for a row's own comparison with a bound: an infinite bound gives an infinite difference, not the NaN of TwoSum's error term
__device__ __forceinline__ double dd_minus(dd t, double b)
{
    const dd s = dd_two_sum(t.hi, -b);
    return isfinite(s.hi) ? s.hi + (s.lo + t.lo) : s.hi;
}
__device__ __forceinline__ dd dd_shfl_xor(dd a, int o) { return {__shfl_xor(a.hi, o, 64), __shfl_xor(a.lo, o, 64)}; }
// butterfly over the lanes whose index differs in the bits [lo_bit, hi_bit): every one of them ends with the same bits
__device__ __forceinline__ dd dd_wave_sum(dd a, int hi_bit, int lo_bit)
{
    for (int o = hi_bit >> 1; o >= lo_bit; o >>= 1) {      // (symmetric in the two partners: TwoSum's error term is exact)
        const dd b = dd_shfl_xor(a, o);
        const dd s = dd_two_sum(a.hi, b.hi);
        a = {s.hi, (a.lo + b.lo) + s.lo};
    }
    return a;
}
__device__ __forceinline__ double cert_nanmax(double a, double b) { return (a != a) ? a : ((b != b) ? b : (a > b ? a : b)); }
__device__ __forceinline__ double cert_wave_nanmax(double v)
{
    for (int o = 32; o > 0; o >>= 1) v = cert_nanmax(v, __shfl_xor(v, o, 64));
    return v;
}

// what the rows of one lane (one row slot, one wave) have shown so far
struct CertRows {
    double pmax, cmax;   // primal, complementarity
    int prow, wrong;
    dd support;
};
__device__ __forceinline__ CertRows cert_rows_init() { return {0.0, 0.0, -1, 0, {0.0, 0.0}}; }
// the larger primal violation; NaN wins, then the smaller row
__device__ __forceinline__ void cert_primal_merge(double &p, int &r, double p2, int r2)
{
    if (p != p) return;
    if (p2 != p2 || p2 > p || (p2 == p && r2 >= 0 && (r < 0 || r2 < r))) { p = p2; r = r2; }
}
// row k with c_k x = cx (a pair): tests/kkt_reference.py:118-147 with q_k = 1
__device__ __forceinline__ void cert_row(CertRows &st, bool active, int k, dd cx, double lam, double bu, double bl, int sense)
{
    if (!active) return;
    const double over = dd_minus(cx, bu), under = -dd_minus(cx, bl);      // > 0: beyond the upper / lower bound
    const bool soft = (sense & kCertSenseSoft) != 0, immutable = (sense & kCertSenseImmutable) != 0;
    const bool equality = immutable && bu == bl, ignored = immutable && !equality;
    const bool nz = lam != 0.0, upper_side = lam > 0.0;
    if (!ignored && !(soft && nz)) {
        const double v = cert_nanmax(over, under);
        if (v > st.pmax || v != v) { if (st.pmax == st.pmax) { st.pmax = v; st.prow = k; } }
    }
    if (equality) st.cmax = cert_nanmax(st.cmax, fabs(over));
    else if (nz && !soft) st.cmax = cert_nanmax(st.cmax, upper_side ? fabs(over) : fabs(under));
    if (nz && !equality) {      // the nearer bound: the sign of 2 c_k x - (bupper_k + blower_k), on pairs (over and under, rounded, may tie where they differ)
        const dd mid = dd_two_sum(bu, bl), s = dd_two_sum(2.0 * cx.hi, -mid.hi);
        const double d = isfinite(s.hi) ? s.hi + ((2.0 * cx.lo - mid.lo) + s.lo) : s.hi;
        if ((d >= 0.0) != upper_side) st.wrong++;
    }
    if (lam > 0.0 || lam < 0.0) {
        dd t = dd_two_prod(lam, upper_side ? bu : bl);
        if (!isfinite(t.hi)) t.lo = 0.0;
        dd_acc(st.support, t);
    }
}

__device__ __forceinline__ void cert_store(const CertifyArgs &a, size_t q, double stat, double hxmax, double fmax_, double rayabs, double rayres,
                                           double pmax, int prow, double cmax, int wrong, double obj, double support)
{
    if (a.stationarity) a.stationarity[q] = stat;
    if (a.stationarity_scale) a.stationarity_scale[q] = cert_nanmax(cert_nanmax(1.0, hxmax), cert_nanmax(fmax_, rayabs));
    if (a.primal) a.primal[q] = pmax;
    if (a.primal_row) a.primal_row[q] = pmax > 0.0 ? prow : -1;
    if (a.complementarity) a.complementarity[q] = cmax;
    if (a.wrong_sign) a.wrong_sign[q] = wrong;
    if (a.objective) a.objective[q] = obj;
    if (a.ray_residual) a.ray_residual[q] = rayres;
    if (a.ray_scale) a.ray_scale[q] = rayabs;
    if (a.ray_support) a.ray_support[q] = support;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// n <= 64: one wavefront per problem
template <int PB>      // problems (waves) per block
__global__ void __launch_bounds__(64 * PB) k_certify_wave(CertifyArgs a)
{
    const int lane = threadIdx.x & 63;
    const size_t q = (size_t)blockIdx.x * PB + (threadIdx.x >> 6);
    if (q >= (size_t)a.N) return;      // (whole waves leave; nothing below synchronises the block)
    const int n = a.n, m = a.m, ms = a.ms, mA = m - ms;
    int W = 1;
    while (W < n) W <<= 1;
    const int col = lane & (W - 1), slot = lane / W, nslots = 64 / W;
    const bool incol = col < n;
    const double *H = a.H ? a.H + (a.shared ? 0 : q * n * n) : nullptr;
    const double *A = mA > 0 ? a.A + (a.shared ? 0 : q * (size_t)mA * n) : nullptr;
    const double *f = a.f + q * n, *x = a.x + q * n, *lam = a.lam + q * m, *bu = a.bupper + q * m, *bl = a.blower + q * m;
    const int *sense = a.sense ? a.sense + q * m : nullptr;

    const double xj = incol ? x[col] : 0.0;
    dd hxf = {0.0, 0.0}, ray = {0.0, 0.0}, rayabs = {0.0, 0.0}, obj = {0.0, 0.0};
    double hxmax = 0.0, fmax_ = 0.0;
    CertRows st = cert_rows_init();

    if (H) {
        double h_next = (slot < n && incol) ? H[(size_t)slot * n + col] : 0.0;
        for (int i0 = 0; i0 < n; i0 += nslots) {
            const int i = i0 + slot, inext = i + nslots;
            const double h = h_next;
            h_next = (inext < n && incol) ? H[(size_t)inext * n + col] : 0.0;
            const dd hx = dd_wave_sum(dd_two_prod(h, xj), W, 1);      // (Hx)_i in every lane of the slot
            if (i < n && col == i) {
                dd_acc(hxf, hx);
                hxmax = cert_nanmax(hxmax, fabs(dd_round(hx)));
                dd t = dd_two_prod(hx.hi, 0.5 * xj);
                t.lo += hx.lo * (0.5 * xj);
                dd_acc(obj, t);
            }
        }
    }
    if (slot == 0 && incol) {
        const double fj = f[col];
        dd_acc(hxf, fj);
        fmax_ = fabs(fj);
        dd_acc(obj, dd_two_prod(fj, xj));
        if (col < ms) {      // simple bound: row col is e_col
            const double l = lam[col];
            dd_acc(ray, l);
            dd_acc(rayabs, fabs(l));
            cert_row(st, true, col, {xj, 0.0}, l, bu[col], bl[col], sense ? sense[col] : 0);
        }
    }
    if (mA > 0) {
        double a_next = (slot < mA && incol) ? A[(size_t)slot * n + col] : 0.0;
        for (int r0 = 0; r0 < mA; r0 += nslots) {
            const int r = r0 + slot, rnext = r + nslots, k = ms + r;
            const bool live = r < mA;
            const double av = a_next;
            a_next = (rnext < mA && incol) ? A[(size_t)rnext * n + col] : 0.0;
            const double l = live ? lam[k] : 0.0;
            const double bu_k = live ? bu[k] : 0.0, bl_k = live ? bl[k] : 0.0;
            const int s_k = (live && sense) ? sense[k] : 0;
            const dd cx = dd_wave_sum(dd_two_prod(av, xj), W, 1);
            dd_acc(ray, dd_two_prod(av, l));
            dd_acc(rayabs, dd_two_prod(av, fabs(l)));
            cert_row(st, live && col == 0, k, cx, l, bu_k, bl_k, s_k);
        }
    }
    // the row slots meet: column sums first (every slot then holds the column's pair)
    hxf = dd_wave_sum(hxf, 64, W);
    ray = dd_wave_sum(ray, 64, W);
    rayabs = dd_wave_sum(rayabs, 64, W);
    dd res = hxf;
    dd_acc(res, ray);
    const double stat = cert_wave_nanmax(fabs(dd_round(res)));
    const double rayres = cert_wave_nanmax(fabs(dd_round(ray)));
    const double rayscale = cert_wave_nanmax(fabs(dd_round(rayabs)));
    hxmax = cert_wave_nanmax(hxmax);
    fmax_ = cert_wave_nanmax(fmax_);
    obj = dd_wave_sum(obj, 64, 1);
    st.support = dd_wave_sum(st.support, 64, 1);
    st.cmax = cert_wave_nanmax(st.cmax);
    for (int o = 32; o > 0; o >>= 1) {
        st.wrong += __shfl_xor(st.wrong, o, 64);
        const double p2 = __shfl_xor(st.pmax, o, 64);
        const int r2 = __shfl_xor(st.prow, o, 64);
        cert_primal_merge(st.pmax, st.prow, p2, r2);
    }
    if (lane == 0) cert_store(a, q, stat, hxmax, fmax_, rayscale, rayres, st.pmax, st.prow, st.cmax, st.wrong, dd_round(obj), dd_round(st.support));
}

// ---------------------------------------------------------------------------------------------------------------------------------
// 65 <= n <= 511: one workgroup per problem, rows dealt to its waves, NC = ceil(n / 64) columns per lane
template <int NC>
__global__ void __launch_bounds__(64 * kCertWaves) k_certify_wg(CertifyArgs a)
{
    extern __shared__ __align__(16) double cert_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t q = blockIdx.x;
    const int n = a.n, m = a.m, ms = a.ms, mA = m - ms;
    const int ncols = (n + 63) / 64 * 64;
    const double *H = a.H ? a.H + (a.shared ? 0 : q * n * n) : nullptr;
    const double *A = mA > 0 ? a.A + (a.shared ? 0 : q * (size_t)mA * n) : nullptr;
    const double *f = a.f + q * n, *x = a.x + q * n, *lam = a.lam + q * m, *bu = a.bupper + q * m, *bl = a.blower + q * m;
    const int *sense = a.sense ? a.sense + q * m : nullptr;

    double xj[NC];
    dd hxf[NC], ray[NC], rayabs[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int col = c * 64 + lane;
        xj[c] = col < n ? x[col] : 0.0;
        hxf[c] = {0.0, 0.0}; ray[c] = {0.0, 0.0}; rayabs[c] = {0.0, 0.0};
    }
    dd obj = {0.0, 0.0};
    double hxmax = 0.0, fmax_ = 0.0;
    CertRows st = cert_rows_init();

    if (H) {
        for (int i = wave; i < n; i += kCertWaves) {
            const double *row = H + (size_t)i * n;
            double h[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) { const int col = c * 64 + lane; h[c] = col < n ? row[col] : 0.0; }
            dd part = {0.0, 0.0};
#pragma unroll
            for (int c = 0; c < NC; ++c) dd_acc(part, dd_two_prod(h[c], xj[c]));
            const dd hx = dd_wave_sum(part, 64, 1);
#pragma unroll
            for (int c = 0; c < NC; ++c)
                if (c * 64 + lane == i) {
                    dd_acc(hxf[c], hx);
                    hxmax = cert_nanmax(hxmax, fabs(dd_round(hx)));
                    dd t = dd_two_prod(hx.hi, 0.5 * xj[c]);
                    t.lo += hx.lo * (0.5 * xj[c]);
                    dd_acc(obj, t);
                }
        }
    }
    if (wave == 0) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int col = c * 64 + lane;
            if (col < n) {
                const double fj = f[col];
                dd_acc(hxf[c], fj);
                fmax_ = cert_nanmax(fmax_, fabs(fj));
                dd_acc(obj, dd_two_prod(fj, xj[c]));
                if (col < ms) {
                    const double l = lam[col];
                    dd_acc(ray[c], l);
                    dd_acc(rayabs[c], fabs(l));
                    cert_row(st, true, col, {xj[c], 0.0}, l, bu[col], bl[col], sense ? sense[col] : 0);
                }
            }
        }
    }
    for (int r = wave; r < mA; r += kCertWaves) {
        const double *row = A + (size_t)r * n;
        const int k = ms + r;
        double av[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) { const int col = c * 64 + lane; av[c] = col < n ? row[col] : 0.0; }
        const double l = lam[k], bu_k = bu[k], bl_k = bl[k];
        const int s_k = sense ? sense[k] : 0;
        dd part = {0.0, 0.0};
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            dd_acc(part, dd_two_prod(av[c], xj[c]));
            dd_acc(ray[c], dd_two_prod(av[c], l));
            dd_acc(rayabs[c], dd_two_prod(av[c], fabs(l)));
        }
        const dd cx = dd_wave_sum(part, 64, 1);
        cert_row(st, lane == 0, k, cx, l, bu_k, bl_k, s_k);
    }

    // ---- the waves meet: column pairs through LDS, added in wave order
    double2 *colbuf = reinterpret_cast<double2 *>(cert_lds);                     // [3][kCertWaves][ncols]
    double *rowbuf = cert_lds + (size_t)3 * kCertWaves * ncols * 2;             // [kCertWaves][16]
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int col = c * 64 + lane;
        if (col < ncols) {
            dd res = hxf[c];
            dd_acc(res, ray[c]);
            colbuf[((size_t)0 * kCertWaves + wave) * ncols + col] = make_double2(res.hi, res.lo);
            colbuf[((size_t)1 * kCertWaves + wave) * ncols + col] = make_double2(ray[c].hi, ray[c].lo);
            colbuf[((size_t)2 * kCertWaves + wave) * ncols + col] = make_double2(rayabs[c].hi, rayabs[c].lo);
        }
    }
    __syncthreads();
    double stat = 0.0, rayres = 0.0, rayscale = 0.0;
    for (int col = threadIdx.x; col < ncols; col += 64 * kCertWaves) {
        dd t[3];
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            const double2 w0 = colbuf[((size_t)v * kCertWaves) * ncols + col];
            t[v] = {w0.x, w0.y};
            for (int w = 1; w < kCertWaves; ++w) {
                const double2 ww = colbuf[((size_t)v * kCertWaves + w) * ncols + col];
                dd_acc(t[v], dd{ww.x, ww.y});
            }
        }
        stat = cert_nanmax(stat, fabs(dd_round(t[0])));
        rayres = cert_nanmax(rayres, fabs(dd_round(t[1])));
        rayscale = cert_nanmax(rayscale, fabs(dd_round(t[2])));
    }
    stat = cert_wave_nanmax(stat);
    rayres = cert_wave_nanmax(rayres);
    rayscale = cert_wave_nanmax(rayscale);
    hxmax = cert_wave_nanmax(hxmax);
    fmax_ = cert_wave_nanmax(fmax_);
    obj = dd_wave_sum(obj, 64, 1);
    st.support = dd_wave_sum(st.support, 64, 1);
    st.cmax = cert_wave_nanmax(st.cmax);
    for (int o = 32; o > 0; o >>= 1) {
        st.wrong += __shfl_xor(st.wrong, o, 64);
        const double p2 = __shfl_xor(st.pmax, o, 64);
        const int r2 = __shfl_xor(st.prow, o, 64);
        cert_primal_merge(st.pmax, st.prow, p2, r2);
    }
    if (lane == 0) {
        double *w = rowbuf + wave * 16;
        w[0] = stat; w[1] = rayres; w[2] = rayscale; w[3] = hxmax; w[4] = fmax_; w[5] = obj.hi; w[6] = obj.lo;
        w[7] = st.support.hi; w[8] = st.support.lo; w[9] = st.cmax; w[10] = st.pmax;
        w[11] = (double)st.prow; w[12] = (double)st.wrong;      // (both far below 2^53: exact)
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w2 = 1; w2 < kCertWaves; ++w2) {
            const double *w = rowbuf + w2 * 16;
            stat = cert_nanmax(stat, w[0]); rayres = cert_nanmax(rayres, w[1]); rayscale = cert_nanmax(rayscale, w[2]);
            hxmax = cert_nanmax(hxmax, w[3]); fmax_ = cert_nanmax(fmax_, w[4]);
            dd_acc(obj, dd{w[5], w[6]});
            dd_acc(st.support, dd{w[7], w[8]});
            st.cmax = cert_nanmax(st.cmax, w[9]);
            cert_primal_merge(st.pmax, st.prow, w[10], (int)w[11]);
            st.wrong += (int)w[12];
        }
        cert_store(a, q, stat, hxmax, fmax_, rayscale, rayres, st.pmax, st.prow, st.cmax, st.wrong, dd_round(obj), dd_round(st.support));
    }
}

extern template __global__ void k_certify_wave<kCertWaves>(CertifyArgs);
extern template __global__ void k_certify_wg<2>(CertifyArgs);
extern template __global__ void k_certify_wg<4>(CertifyArgs);
extern template __global__ void k_certify_wg<8>(CertifyArgs);

} // namespace daqp_amd
