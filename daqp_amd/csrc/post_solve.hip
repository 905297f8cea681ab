// post_solve.hip -- host side of the calls that run behind a solve: the adjoint (daqp_batch_backward*), the refinement
// (daqp_batch_refine, daqp_batch_refine_nullspace) and the certificate (daqp_certify_batch).  Each is argument checks, one or two
// launches and the three helpers below; the kernels are in backward_kernel.hip, refine_kernel.hip and certify_kernel.hip.
#include <cstring>

#define DAQP_AMD_PLAN_TYPES_ONLY   // (this unit reads plans; the planner's kernel headers belong to daqp_amd.hip)
#include "host.hip.h"
#include "backward.hip.h"
#include "nullspace.hip.h"
#include "certify.hip.h"
#include "refine.hip.h"
#include "refine_nullspace.hip.h"
#include "eliminate.hip.h"
#include "eliminate_adjoint.hip.h"

namespace daqp_amd {
// the adjoint kernel: backward_kernel.hip
extern template __global__ void k_backward<64, true, true, false>(BatchDev, BackwardArgs);
extern template __global__ void k_backward<256, false, true, false>(BatchDev, BackwardArgs);
extern template __global__ void k_backward<256, false, false, false>(BatchDev, BackwardArgs);
extern template __global__ void k_backward<64, true, true, true>(BatchDev, BackwardArgs);
extern template __global__ void k_backward<256, false, true, true>(BatchDev, BackwardArgs);
extern template __global__ void k_backward<256, false, false, true>(BatchDev, BackwardArgs);
extern template __global__ void k_backward<64, true, true, false, true>(BatchDev, BackwardArgs);
extern template __global__ void k_backward<256, false, true, false, true>(BatchDev, BackwardArgs);
extern template __global__ void k_backward<256, false, false, false, true>(BatchDev, BackwardArgs);
extern template __global__ void k_backward<64, true, true, true, true>(BatchDev, BackwardArgs);
extern template __global__ void k_backward<256, false, true, true, true>(BatchDev, BackwardArgs);
extern template __global__ void k_backward<256, false, false, true, true>(BatchDev, BackwardArgs);
extern template __global__ void k_backward_nullspace<64>(BatchDev, NullspaceArgs);
extern template __global__ void k_backward_nullspace<64, true>(BatchDev, NullspaceArgs);
// the elimination kernels: eliminate_kernel.hip
extern template __global__ void k_eliminate<1, 1>(ElimDev);
extern template __global__ void k_eliminate<2, 4>(ElimDev);
extern template __global__ void k_eliminate<4, 4>(ElimDev);
extern template __global__ void k_eliminate<8, 4>(ElimDev);
extern template __global__ void k_eliminate_update<1>(ElimDev);
extern template __global__ void k_eliminate_update<2>(ElimDev);
extern template __global__ void k_eliminate_update<4>(ElimDev);
extern template __global__ void k_eliminate_update<8>(ElimDev);
extern template __global__ void k_expand<1>(ElimDev, ExpandArgs);
extern template __global__ void k_expand<2>(ElimDev, ExpandArgs);
extern template __global__ void k_expand<4>(ElimDev, ExpandArgs);
extern template __global__ void k_expand<8>(ElimDev, ExpandArgs);
extern template __global__ void k_elim_basis<1>(ElimDev, double *);
extern template __global__ void k_elim_basis<2>(ElimDev, double *);
extern template __global__ void k_elim_basis<4>(ElimDev, double *);
extern template __global__ void k_elim_basis<8>(ElimDev, double *);
extern template __global__ void k_adjoint_reduce<1>(ElimDev, ElimAdjointArgs);
extern template __global__ void k_adjoint_reduce<2>(ElimDev, ElimAdjointArgs);
extern template __global__ void k_adjoint_reduce<4>(ElimDev, ElimAdjointArgs);
extern template __global__ void k_adjoint_reduce<8>(ElimDev, ElimAdjointArgs);
extern template __global__ void k_adjoint_expand<1>(ElimDev, ElimAdjointArgs);
extern template __global__ void k_adjoint_expand<2>(ElimDev, ElimAdjointArgs);
extern template __global__ void k_adjoint_expand<4>(ElimDev, ElimAdjointArgs);
extern template __global__ void k_adjoint_expand<8>(ElimDev, ElimAdjointArgs);
}

// What daqp_batch_eliminate keeps: the caller's problem (device pointers: borrowed, or the handle's own copies of host arrays), the
// factor Q, R of the equality rows, x0, c0, the flags and the reduced problem -- everything on one device, launched on one stream.
struct DAQPBatchElimination {
    int device = 0;
    hipStream_t stream = nullptr;
    daqp_amd::ElimDev d{};
    std::vector<void *> owned;
    unsigned long long bytes = 0;
    double *own_f = nullptr, *own_bu = nullptr, *own_bl = nullptr;      // the handle's copies of host-resident f / bounds
    int grid = 0;      // workgroup tier: persistent blocks, one n x n scratch matrix each
    // daqp_batch_eliminate_backward's intermediates, allocated by its first call: grad_y, dz_r [N][nr], grad_lam_r, dbupper_r,
    // dblower_r [N][mr], dz0 [N][n], status_r [N]
    double *adj_gy = nullptr, *adj_glr = nullptr, *adj_dz0 = nullptr, *adj_dzr = nullptr, *adj_dbur = nullptr, *adj_dblr = nullptr;
    int *adj_str = nullptr;
};

using namespace daqp_amd;

namespace {

// ---- which instantiation of a kernel with the adjoint's tiers: one wavefront with everything in LDS (n <= 64, and the cap rows of
// the working set and their Gram matrix fit), a workgroup with rows + Gram matrix in LDS, or in scratch.  fits == false: not even that.
struct Tier { bool small, nl, fits; size_t lds; int block; };
Tier pick_tier(int n, int cap, size_t (*lds_bytes)(int, int, bool, bool))
{
    const size_t lds_max = (size_t)144 * 1024;
    const bool small = n <= 64 && lds_bytes(n, cap, true, true) <= lds_max;
    const size_t lds_nl = lds_bytes(n, cap, small, true);
    const bool nl = small || lds_nl <= lds_max;
    const size_t lds = nl ? lds_nl : lds_bytes(n, cap, false, false);
    return {small, nl, lds <= lds_max, lds, small ? 64 : 256};
}

// ---- the grid of a launch whose rows live in scratch (allocated with the family's first such call): persistent workgroups, at most
// 512 of them and at most 256 MiB of scratch.  0: the allocation failed.
int scratch_grid(DAQPBatch *b, PostSolveBufs &f, size_t scratch_per_wg)
{
    if (!f.scratch) {
        size_t g = ((size_t)256 << 20) / (scratch_per_wg * sizeof(double));
        if (g > 512) g = 512;
        if (g < 16) g = 16;
        if (g > (size_t)b->d.N) g = b->d.N;
        if (dev_alloc(b, &f.scratch, g * scratch_per_wg)) return 0;
        f.grid = (int)g;
    }
    return f.grid;
}

// ---- the arguments of one call, as the kernel gets them.  Device-resident ones are used in place: no copy, and finish() waits for nothing.
// Host-resident ones get a device slot each -- the batch's own (kept for the next call) or the call's (freed on return) --, allocated when first
// needed: a failed allocation leaves the ones before it in place.  finish() copies the outputs back in the order they were declared and waits once.
struct Staging {
    DAQPBatch *const b;
    const hipStream_t s;
    const bool device;           // the arguments are device-resident
    void *local[18] = {};        // the call's own slots
    void **const slots;
    struct Back { void *host; const void *dev; size_t bytes; } back[18];      // what finish() copies back
    int n_back = 0;
    Staging(DAQPBatch *b, void **slots, hipStream_t s, int memory) : b(b), s(s), device(memory == DAQP_MEM_DEVICE), slots(slots ? slots : local) {}
    ~Staging() { for (void *p : local) if (p) (void)hipFree(p); }
    template <typename T>
    int arg(T **dev, int slot, T *host, size_t count, bool copy_in, bool copy_back)
    {
        *dev = host;                                   // (a null host pointer gives a null device pointer)
        if (device || !host) return 0;
        T **p = reinterpret_cast<T **>(&slots[slot]);
        if (!*p) {
            if (slots != local) { if (dev_alloc(b, p, count)) return DAQP_EXIT_UNSUPPORTED; }
            else HIPCHK(hipMalloc(reinterpret_cast<void **>(p), (count ? count : 1) * sizeof(T)));
        }
        *dev = *p;
        if (copy_in && count) HIPCHK(hipMemcpyAsync(*p, host, count * sizeof(T), hipMemcpyHostToDevice, s));
        if (copy_back) back[n_back++] = {host, *p, count * sizeof(T)};
        return 0;
    }
    template <typename T> int in(const T **dev, int slot, const T *host, size_t count) { return arg(const_cast<T **>(dev), slot, const_cast<T *>(host), count, true, false); }
    template <typename T> int out(T **dev, int slot, T *host, size_t count) { return arg(dev, slot, host, count, false, true); }
    template <typename T> int inout(T **dev, int slot, T *host, size_t count) { return arg(dev, slot, host, count, true, true); }
    int finish()
    {
        if (device) return 0;
        for (int i = 0; i < n_back; ++i)
            if (back[i].bytes) HIPCHK(hipMemcpyAsync(back[i].host, back[i].dev, back[i].bytes, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        return 0;
    }
};

// The adjoint of the last solve (include/daqp_amd.h, backward.hip.h): one launch on the batch's stream.  Refusals come before any
// device work.  Host-resident arguments go through the batch's own staging buffers and the call waits for the results; device-resident
// ones are used in place and nothing waits.  Batches created with ns_max > 0 run the SOFT instantiations (soft rows in the (2,2)
// block, q_k / u_k emitted where asked for); every other batch runs the kernels it ran before there were any.
// nsw: the null-space kernel (nullspace.hip.h) on the same stream -- -1: not at all; 0: behind k_backward, for the problems that went
// through the proximal loop only (it overwrites their outputs; every other problem keeps k_backward's bits); 1: instead of k_backward,
// for every problem.  Launched for n <= 64 only: beyond, nsw == 0 leaves k_backward's DAQP_EXIT_UNSUPPORTED and nsw == 1 was refused.
// grad_lam != null (daqp_batch_backward_dual, ns_max == 0 only): the DUAL instantiations of both kernels -- g_lam on W in the second
// block of the right-hand side -- with the same tiers (they need no LDS of their own: backward_lds_bytes is unchanged); grad_x may then be null.
// soft_dual (daqp_batch_backward_soft_dual, ns_max > 0 only): the SOFT && DUAL instantiations -- grad_lam and / or grad_slack (with the
// lam of the solve) in the second block; each of the two may be null.  Their LDS is that of the SOFT ones (ghat_lam lives in y[], which
// the SOFT and the DUAL kernels both carry and leave idle until the triangular solves), so the tier pick is the same function of (n, cap).
int backward_launch(const char *who, DAQPBatch *b, const c_float *grad_x, c_float *dz, c_float *dbupper, c_float *dblower,
                    c_float *qsoft, c_float *usoft, int *usoft_id, int *status, int memory, int nsw = -1, const c_float *grad_lam = nullptr,
                    bool soft_dual = false, const c_float *grad_slack = nullptr, const c_float *lam = nullptr)
{
    if (!b->is_setup || !b->solved || b->pending_mask) {
        set_err("%s: the last operation on the batch was not a successful daqp_batch_solve", who);
        return DAQP_EXIT_UNSUPPORTED;
    }
    HIPCHK(hipSetDevice(b->device));
    const BatchDev &d = b->d;
    const size_t N = d.N, n = d.n, m = d.m, ns = b->plan.ns_max;
    const bool soft = b->plan.ns_max > 0;
    if (!soft) qsoft = nullptr, usoft = nullptr, usoft_id = nullptr;      // (ns_max == 0: usoft / usoft_id are empty, qsoft is zeroed by the entry)
    const Tier t = pick_tier(d.n, d.cap, backward_lds_bytes);
    if (!t.fits && nsw != 1) { set_err("%s: n = %d with working sets of %d rows does not fit the adjoint kernel", who, d.n, d.cap); return DAQP_EXIT_UNSUPPORTED; }
    void (*kb)(BatchDev, BackwardArgs);
    if (soft && soft_dual) kb = t.small ? k_backward<64, true, true, true, true> : (t.nl ? k_backward<256, false, true, true, true> : k_backward<256, false, false, true, true>);
    else if (soft) kb = t.small ? k_backward<64, true, true, true> : (t.nl ? k_backward<256, false, true, true> : k_backward<256, false, false, true>);
    else if (grad_lam) kb = t.small ? k_backward<64, true, true, false, true> : (t.nl ? k_backward<256, false, true, false, true> : k_backward<256, false, false, false, true>);
    else kb = t.small ? k_backward<64, true, true, false> : (t.nl ? k_backward<256, false, true, false> : k_backward<256, false, false, false>);
    BackwardArgs a{};
    int grid = d.N;
    if (!t.nl && nsw != 1) {
        a.scratch_per_wg = backward_scratch_doubles(d.n, d.cap);
        if (!(grid = scratch_grid(b, b->adjoint, a.scratch_per_wg))) return DAQP_EXIT_UNSUPPORTED;
        a.scratch = b->adjoint.scratch;
    }
    Staging st(b, b->adjoint.slot, b->stream, memory);
    if (st.in(&a.grad_x, 0, grad_x, N * n) || st.out(&a.dz, 1, dz, N * n) || st.out(&a.dbupper, 2, dbupper, N * m) ||
        st.out(&a.dblower, 3, dblower, N * m) || st.out(&a.qsoft, 4, qsoft, N * m) || st.out(&a.usoft, 5, usoft, N * ns * n) ||
        st.out(&a.usoft_id, 6, usoft_id, N * ns) || st.out(&a.status, 7, status, N) || st.in(&a.grad_lam, 8, grad_lam, N * m) ||
        st.in(&a.grad_slack, 9, grad_slack, N) || st.in(&a.lam, 10, lam, N * m))
        return DAQP_EXIT_UNSUPPORTED;
    if (nsw != 1) {
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(kb), hipFuncAttributeMaxDynamicSharedMemorySize, (int)t.lds));
        hipLaunchKernelGGL(kb, dim3(grid), dim3(t.block), t.lds, b->stream, d, a);
        HIPCHK(hipGetLastError());
    }
    if (nsw >= 0 && d.n <= 64) {
        NullspaceArgs na{};
        na.grad_x = a.grad_x; na.dz = a.dz; na.dbupper = a.dbupper; na.dblower = a.dblower; na.status = a.status;
        na.lp = (b->ident && d.H == b->ident) ? 1 : 0;
        na.only_prox = nsw == 0 ? 1 : 0;
        na.grad_lam = a.grad_lam;
        void (*kn)(BatchDev, NullspaceArgs) = grad_lam ? k_backward_nullspace<64, true> : k_backward_nullspace<64>;
        const size_t lds_ns = nullspace_lds_bytes(d.n);
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(kn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_ns));
        hipLaunchKernelGGL(kn, dim3(d.N), dim3(64), lds_ns, b->stream, d, na);
        HIPCHK(hipGetLastError());
    }
    return st.finish();
}

// Iterative refinement of (x, lam) at the stored working set (include/daqp_amd.h, refine.hip.h): one launch on the batch's stream.
// Refusals come before any device work.  Host-resident arguments go through the batch's own staging buffers and the call waits for
// the results; device-resident ones are used in place and nothing waits.  Nothing of the batch's state is written.
// nsw: the null-space kernel (refine_nullspace.hip.h) on the same stream -- -1: not at all; 0: behind k_refine, for the problems that
// went through the proximal loop only (it overwrites their outputs; every other problem keeps k_refine's bits); 1: instead of
// k_refine, for every problem.  Launched for n <= 64 only: beyond, nsw == 0 leaves k_refine's DAQP_EXIT_UNSUPPORTED and nsw == 1 was refused.
int refine_launch(const char *who, DAQPBatch *b, c_float *x, c_float *lam, c_float *fval, c_float *residual, int *steps, int *status,
                  int max_steps, int memory, int nsw = -1)
{
    if (!b || !x || !lam || !status) { set_err("%s: null batch, x, lam or status", who); return DAQP_EXIT_UNSUPPORTED; }
    if (b->plan.ns_max > 0) { set_err("%s: batches created with ns_max > 0 (soft constraints) are not supported: soft rows change the (2,2) block of the system", who); return DAQP_EXIT_UNSUPPORTED; }
    if (max_steps < 1 || max_steps > kRefineMaxSteps) { set_err("%s: max_steps must be in 1..%d (got %d)", who, kRefineMaxSteps, max_steps); return DAQP_EXIT_UNSUPPORTED; }
    if (memory != DAQP_MEM_HOST && memory != DAQP_MEM_DEVICE) { set_err("%s: memory must be DAQP_MEM_HOST or DAQP_MEM_DEVICE", who); return DAQP_EXIT_UNSUPPORTED; }
    if (nsw == 1 && b->d.n > 64) { set_err("%s: which == 1 needs n <= 64 (n = %d): the null-space kernel holds a problem in one wavefront", who, b->d.n); return DAQP_EXIT_UNSUPPORTED; }
    if (!b->is_setup || !b->solved || b->pending_mask) {
        set_err("%s: the last operation on the batch was not a successful daqp_batch_solve", who);
        return DAQP_EXIT_UNSUPPORTED;
    }
    const BatchDev &d = b->d;
    if (!d.H || !d.f || !d.bu || !d.bl || (d.mA > 0 && !d.A)) { set_err("%s: the batch has no H, f, A or bounds of the caller's to read", who); return DAQP_EXIT_UNSUPPORTED; }
    HIPCHK(hipSetDevice(b->device));
    const size_t N = d.N, n = d.n, m = d.m;
    const Tier t = pick_tier(d.n, d.cap, refine_lds_bytes);
    if (!t.fits && nsw != 1) { set_err("%s: n = %d with working sets of %d rows does not fit the refinement kernel", who, d.n, d.cap); return DAQP_EXIT_UNSUPPORTED; }
    void (*kr)(BatchDev, RefineArgs) = t.small ? k_refine<64, true, true> : (t.nl ? k_refine<256, false, true> : k_refine<256, false, false>);
    RefineArgs a{};
    a.max_steps = max_steps;
    int grid = d.N;
    if (!t.nl && nsw != 1) {
        a.scratch_per_wg = refine_scratch_doubles(d.n, d.cap);
        if (!(grid = scratch_grid(b, b->refine, a.scratch_per_wg))) return DAQP_EXIT_UNSUPPORTED;
        a.scratch = b->refine.scratch;
    }
    Staging st(b, b->refine.slot, b->stream, memory);
    if (st.inout(&a.x, 0, x, N * n) || st.inout(&a.lam, 1, lam, N * m) || st.inout(&a.fval, 2, fval, N) ||      // (fval: untouched where the status is not 0)
        st.out(&a.residual, 3, residual, 2 * N) || st.out(&a.steps, 4, steps, N) || st.out(&a.status, 5, status, N))
        return DAQP_EXIT_UNSUPPORTED;
    if (nsw != 1) {
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(kr), hipFuncAttributeMaxDynamicSharedMemorySize, (int)t.lds));
        hipLaunchKernelGGL(kr, dim3(grid), dim3(t.block), t.lds, b->stream, d, a);
        HIPCHK(hipGetLastError());
    }
    if (nsw >= 0 && d.n <= 64) {
        RefineNullspaceArgs na{};
        na.r = a; na.r.scratch = nullptr; na.r.scratch_per_wg = 0;
        na.lp = (b->ident && d.H == b->ident) ? 1 : 0;
        na.only_prox = nsw == 0 ? 1 : 0;
        const size_t lds_ns = nullspace_lds_bytes(d.n);
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_refine_nullspace<64>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_ns));
        hipLaunchKernelGGL(k_refine_nullspace<64>, dim3(d.N), dim3(64), lds_ns, b->stream, d, na);
        HIPCHK(hipGetLastError());
    }
    return st.finish();
}

int certify_launch(const CertifyArgs &a, hipStream_t s)
{
    if (a.n <= 64) {
        hipLaunchKernelGGL(k_certify_wave<kCertWaves>, dim3((a.N + kCertWaves - 1) / kCertWaves), dim3(64 * kCertWaves), 0, s, a);
    } else {
        void (*k)(CertifyArgs) = a.n <= 128 ? k_certify_wg<2> : (a.n <= 256 ? k_certify_wg<4> : k_certify_wg<8>);
        const size_t lds = certify_wg_lds_bytes(a.n);
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k, dim3(a.N), dim3(64 * kCertWaves), lds, s, a);
    }
    HIPCHK(hipGetLastError());
    return 0;
}
// (stateless: the device copies of host-resident arguments are the call's own and gone when it returns)
int certify_run(DAQPBatchCertificate *out, const DAQPBatchProblem *p, const c_float *x, const c_float *lam, int shared, hipStream_t s)
{
    const size_t N = p->N, n = p->n, m = p->m, mA = p->m - p->ms, nm = shared ? 1 : N;
    CertifyArgs a{};
    a.N = p->N; a.n = p->n; a.m = p->m; a.ms = p->ms; a.shared = shared ? 1 : 0;
    Staging st(nullptr, nullptr, s, p->memory);
    if (st.in(&a.H, 0, p->H, nm * n * n) || st.in(&a.f, 1, p->f, N * n) || st.in(&a.A, 2, p->A, nm * mA * n) ||
        st.in(&a.bupper, 3, p->bupper, N * m) || st.in(&a.blower, 4, p->blower, N * m) || st.in(&a.sense, 5, p->sense, N * m) ||
        st.in(&a.x, 6, x, N * n) || st.in(&a.lam, 7, lam, N * m))
        return DAQP_EXIT_UNSUPPORTED;
    if (st.out(&a.stationarity, 8, out->stationarity, N) || st.out(&a.stationarity_scale, 9, out->stationarity_scale, N) ||
        st.out(&a.primal, 10, out->primal, N) || st.out(&a.complementarity, 11, out->complementarity, N) || st.out(&a.objective, 12, out->objective, N) ||
        st.out(&a.ray_residual, 13, out->ray_residual, N) || st.out(&a.ray_scale, 14, out->ray_scale, N) || st.out(&a.ray_support, 15, out->ray_support, N) ||
        st.out(&a.wrong_sign, 16, out->wrong_sign, N) || st.out(&a.primal_row, 17, out->primal_row, N))
        return DAQP_EXIT_UNSUPPORTED;
    if (certify_launch(a, s)) return DAQP_EXIT_UNSUPPORTED;
    return st.finish();
}

// ---- equality elimination (include/daqp_amd.h, eliminate.hip.h)
template <typename T>
int elim_alloc(DAQPBatchElimination *el, T **p, size_t count, bool zero = false)
{
    if (count == 0) count = 1;
    HIPCHK(hipMalloc(reinterpret_cast<void **>(p), count * sizeof(T)));
    el->owned.push_back(*p);
    el->bytes += count * sizeof(T);
    if (zero) HIPCHK(hipMemsetAsync(*p, 0, count * sizeof(T), el->stream));
    return 0;
}
// a device copy of a host array in a buffer of the handle's (allocated when first needed)
template <typename T>
int elim_copy(DAQPBatchElimination *el, T **own, const T *host, size_t count)
{
    if (!*own && elim_alloc(el, own, count)) return DAQP_EXIT_UNSUPPORTED;
    HIPCHK(hipMemcpyAsync(*own, host, count * sizeof(T), hipMemcpyHostToDevice, el->stream));
    return 0;
}
bool elim_no_device(int *ndev)
{
    *ndev = 0;
    if (hipGetDeviceCount(ndev) != hipSuccess || *ndev == 0) {
        set_err("no HIP device: libdaqp_amd has no CPU path");
        return true;
    }
    return false;
}
template <typename K1, typename K2, typename K4, typename K8>
auto elim_pick(int n, K1 k1, K2 k2, K4 k4, K8 k8) { const int nv = elim_nv(n); return nv == 1 ? k1 : (nv == 2 ? k2 : (nv == 4 ? k4 : k8)); }

int elim_run(DAQPBatchElimination *el)
{
    const ElimDev &d = el->d;
    // the tier is decided by n alone: one wavefront with H and the reflectors in LDS (69.1 KB at most), a workgroup of four beyond
    const bool wave = d.n <= 64;
    const size_t lds = elim_lds_bytes(d.n, d.neq, wave);
    void (*k)(ElimDev) = elim_pick(d.n, k_eliminate<1, 1>, k_eliminate<2, 4>, k_eliminate<4, 4>, k_eliminate<8, 4>);
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k, dim3(wave ? d.N : el->grid), dim3(wave ? 64 : 256), lds, el->stream, d);
    HIPCHK(hipGetLastError());
    return 0;
}

} // namespace

extern "C" {

// ---- equality elimination: argument checks first, then the device, then the work.  A failed daqp_batch_eliminate leaves no handle.
int daqp_batch_eliminate(DAQPBatchElimination **out, const DAQPBatchProblem *p, const int *eq_rows, int neq,
                         const DAQPSettings *settings, int device, void *hip_stream)
{
    int ndev = 0;
    if (out) *out = nullptr;
    if (elim_no_device(&ndev)) return DAQP_EXIT_UNSUPPORTED;
    if (!out || !p || !eq_rows) { set_err("daqp_batch_eliminate: null out, problem or eq_rows"); return DAQP_EXIT_UNSUPPORTED; }
    if (p->N <= 0 || p->n <= 0 || p->m < 0 || p->m > (1 << 24) || p->ms < 0 || p->ms > p->n || p->ms > p->m) {
        set_err("daqp_batch_eliminate: bad dimensions N=%d n=%d m=%d ms=%d (N >= 1, n >= 1, 0 <= m <= 2^24, ms <= n, ms <= m)", p->N, p->n, p->m, p->ms);
        return DAQP_EXIT_UNSUPPORTED;
    }
    if (p->n > 511) { set_err("daqp_batch_eliminate: n = %d: the elimination kernels take n <= 511", p->n); return DAQP_EXIT_UNSUPPORTED; }
    if (neq < 1 || neq >= p->n) { set_err("daqp_batch_eliminate: neq = %d must be in 1..n-1 (n = %d)", neq, p->n); return DAQP_EXIT_UNSUPPORTED; }
    for (int c = 0; c < neq; ++c) {
        if (eq_rows[c] < 0 || eq_rows[c] >= p->m) { set_err("daqp_batch_eliminate: eq_rows[%d] = %d is out of range 0..%d", c, eq_rows[c], p->m - 1); return DAQP_EXIT_UNSUPPORTED; }
        if (c > 0 && eq_rows[c] <= eq_rows[c - 1]) { set_err("daqp_batch_eliminate: eq_rows must be distinct and ascending (eq_rows[%d] = %d after %d)", c, eq_rows[c], eq_rows[c - 1]); return DAQP_EXIT_UNSUPPORTED; }
    }
    if (!p->f || (p->m > p->ms && !p->A) || !p->bupper || !p->blower) { set_err("daqp_batch_eliminate: null f, A or bounds"); return DAQP_EXIT_UNSUPPORTED; }
    if (p->memory != DAQP_MEM_HOST && p->memory != DAQP_MEM_DEVICE) { set_err("daqp_batch_eliminate: memory must be DAQP_MEM_HOST or DAQP_MEM_DEVICE"); return DAQP_EXIT_UNSUPPORTED; }
    if (device < 0) { if (hipGetDevice(&device) != hipSuccess) device = 0; }
    if (device >= ndev) { set_err("daqp_batch_eliminate: device %d of %d", device, ndev); return DAQP_EXIT_UNSUPPORTED; }
    HIPCHK(hipSetDevice(device));
    if (device < 64) g_devices_used.fetch_or(1ull << device);
    DAQPSettings st;
    if (settings) st = *settings; else daqp_default_settings(&st);

    std::unique_ptr<DAQPBatchElimination, void (*)(DAQPBatchElimination *)> el(new DAQPBatchElimination, daqp_batch_elimination_free);
    el->device = device;
    el->stream = reinterpret_cast<hipStream_t>(hip_stream);
    ElimDev &d = el->d;
    d.N = p->N; d.n = p->n; d.m = p->m; d.ms = p->ms; d.neq = neq; d.nr = p->n - neq; d.mr = p->m - neq; d.ldn = p->n | 1;
    d.lp = p->H ? 0 : 1;
    d.zero_tol = st.zero_tol;
    const size_t N = d.N, n = d.n, m = d.m, mA = d.m - d.ms, nr = d.nr, mr = d.mr;
    std::vector<int> kept;
    for (int r = 0, c = 0; r < d.m; ++r) {
        if (c < neq && eq_rows[c] == r) ++c;
        else kept.push_back(r);
    }
    int *rows_dev = nullptr, *kept_dev = nullptr;
    if (elim_alloc(el.get(), &rows_dev, neq) || elim_alloc(el.get(), &kept_dev, mr)) return DAQP_EXIT_UNSUPPORTED;
    HIPCHK(hipMemcpy(rows_dev, eq_rows, sizeof(int) * neq, hipMemcpyHostToDevice));
    if (mr) HIPCHK(hipMemcpy(kept_dev, kept.data(), sizeof(int) * mr, hipMemcpyHostToDevice));
    d.eq_rows = rows_dev; d.kept = kept_dev;
    if (p->memory == DAQP_MEM_DEVICE) {
        d.H = p->H; d.f = p->f; d.A = p->A; d.bu = p->bupper; d.bl = p->blower; d.sense = p->sense;
    } else {
        double *H = nullptr, *A = nullptr; int *sense = nullptr;
        if (p->H && elim_copy(el.get(), &H, p->H, N * n * n)) return DAQP_EXIT_UNSUPPORTED;
        if (mA && elim_copy(el.get(), &A, p->A, N * mA * n)) return DAQP_EXIT_UNSUPPORTED;
        if (p->sense && elim_copy(el.get(), &sense, p->sense, N * m)) return DAQP_EXIT_UNSUPPORTED;
        if (elim_copy(el.get(), &el->own_f, p->f, N * n) || elim_copy(el.get(), &el->own_bu, p->bupper, N * m) || elim_copy(el.get(), &el->own_bl, p->blower, N * m))
            return DAQP_EXIT_UNSUPPORTED;
        d.H = H; d.A = A; d.sense = sense; d.f = el->own_f; d.bu = el->own_bu; d.bl = el->own_bl;
    }
    if (elim_alloc(el.get(), &d.V, N * neq * d.ldn, true) || elim_alloc(el.get(), &d.beta, N * neq) || elim_alloc(el.get(), &d.rd, N * neq) ||
        elim_alloc(el.get(), &d.rn, N * neq) || elim_alloc(el.get(), &d.x0, N * n) || elim_alloc(el.get(), &d.c0, N) || elim_alloc(el.get(), &d.flags, N) ||
        elim_alloc(el.get(), &d.Hr, d.lp ? 1 : N * nr * nr) || elim_alloc(el.get(), &d.fr, N * nr) || elim_alloc(el.get(), &d.Ar, N * mr * nr) ||
        elim_alloc(el.get(), &d.bur, N * mr) || elim_alloc(el.get(), &d.blr, N * mr) || elim_alloc(el.get(), &d.senser, N * mr))
        return DAQP_EXIT_UNSUPPORTED;
    if (d.n > 64) {      // persistent workgroups, at most 512 of them and at most 256 MiB of scratch (post-solve's scratch_grid rule)
        size_t g = ((size_t)256 << 20) / (n * n * sizeof(double));
        if (g > 512) g = 512;
        if (g < 16) g = 16;
        if (g > N) g = N;
        if (elim_alloc(el.get(), &d.scratch, g * n * n)) return DAQP_EXIT_UNSUPPORTED;
        el->grid = (int)g;
    }
    if (elim_run(el.get())) return DAQP_EXIT_UNSUPPORTED;
    if (p->memory == DAQP_MEM_HOST) HIPCHK(hipStreamSynchronize(el->stream));      // the host arrays are the caller's again
    *out = el.release();
    return 0;
}

int daqp_batch_eliminate_update(DAQPBatchElimination *el, const c_float *f, const c_float *bupper, const c_float *blower, int memory)
{
    int ndev = 0;
    if (elim_no_device(&ndev)) return DAQP_EXIT_UNSUPPORTED;
    if (!el) { set_err("daqp_batch_eliminate_update: null handle"); return DAQP_EXIT_UNSUPPORTED; }
    if (memory != DAQP_MEM_HOST && memory != DAQP_MEM_DEVICE) { set_err("daqp_batch_eliminate_update: memory must be DAQP_MEM_HOST or DAQP_MEM_DEVICE"); return DAQP_EXIT_UNSUPPORTED; }
    HIPCHK(hipSetDevice(el->device));
    ElimDev &d = el->d;
    const size_t N = d.N, n = d.n, m = d.m;
    if (memory == DAQP_MEM_DEVICE) {
        if (f) d.f = f;
        if (bupper) d.bu = bupper;
        if (blower) d.bl = blower;
    } else {
        if (f) { if (elim_copy(el, &el->own_f, f, N * n)) return DAQP_EXIT_UNSUPPORTED; d.f = el->own_f; }
        if (bupper) { if (elim_copy(el, &el->own_bu, bupper, N * m)) return DAQP_EXIT_UNSUPPORTED; d.bu = el->own_bu; }
        if (blower) { if (elim_copy(el, &el->own_bl, blower, N * m)) return DAQP_EXIT_UNSUPPORTED; d.bl = el->own_bl; }
    }
    void (*k)(ElimDev) = elim_pick(d.n, k_eliminate_update<1>, k_eliminate_update<2>, k_eliminate_update<4>, k_eliminate_update<8>);
    hipLaunchKernelGGL(k, dim3(d.N), dim3(64), 0, el->stream, d);
    HIPCHK(hipGetLastError());
    if (memory == DAQP_MEM_HOST) HIPCHK(hipStreamSynchronize(el->stream));
    return 0;
}

int daqp_batch_elimination_problem(DAQPBatchElimination *el, DAQPBatchProblem *reduced)
{
    int ndev = 0;
    if (elim_no_device(&ndev)) return DAQP_EXIT_UNSUPPORTED;
    if (!el || !reduced) { set_err("daqp_batch_elimination_problem: null handle or problem"); return DAQP_EXIT_UNSUPPORTED; }
    const ElimDev &d = el->d;
    reduced->N = d.N; reduced->n = d.nr; reduced->m = d.mr; reduced->ms = 0;
    reduced->H = d.lp ? nullptr : d.Hr; reduced->f = d.fr; reduced->A = d.Ar; reduced->bupper = d.bur; reduced->blower = d.blr;
    reduced->sense = d.senser;
    reduced->memory = DAQP_MEM_DEVICE;
    return 0;
}

int daqp_batch_elimination_flags(DAQPBatchElimination *el, int *flags_host)
{
    int ndev = 0;
    if (elim_no_device(&ndev)) return DAQP_EXIT_UNSUPPORTED;
    if (!el || !flags_host) { set_err("daqp_batch_elimination_flags: null handle or array"); return DAQP_EXIT_UNSUPPORTED; }
    HIPCHK(hipSetDevice(el->device));
    HIPCHK(hipMemcpyAsync(flags_host, el->d.flags, sizeof(int) * el->d.N, hipMemcpyDeviceToHost, el->stream));
    HIPCHK(hipStreamSynchronize(el->stream));
    return 0;
}

int daqp_batch_expand(DAQPBatchElimination *el, const DAQPBatchResult *reduced, DAQPBatchResult *full)
{
    int ndev = 0;
    if (elim_no_device(&ndev)) return DAQP_EXIT_UNSUPPORTED;
    if (!el || !reduced || !full) { set_err("daqp_batch_expand: null handle or result"); return DAQP_EXIT_UNSUPPORTED; }
    if (!reduced->x || !reduced->lam || !reduced->exitflag) { set_err("daqp_batch_expand: null x, lam or exitflag in the reduced result"); return DAQP_EXIT_UNSUPPORTED; }
    if ((reduced->memory != DAQP_MEM_HOST && reduced->memory != DAQP_MEM_DEVICE) || (full->memory != DAQP_MEM_HOST && full->memory != DAQP_MEM_DEVICE)) {
        set_err("daqp_batch_expand: memory must be DAQP_MEM_HOST or DAQP_MEM_DEVICE");
        return DAQP_EXIT_UNSUPPORTED;
    }
    if (reduced->memory != full->memory) { set_err("daqp_batch_expand: host and device memory mixed in one call (reduced and full results must live on the same side)"); return DAQP_EXIT_UNSUPPORTED; }
    HIPCHK(hipSetDevice(el->device));
    const ElimDev &d = el->d;
    const size_t N = d.N, n = d.n, m = d.m, nr = d.nr, mr = d.mr;
    ExpandArgs a{};
    Staging st(nullptr, nullptr, el->stream, full->memory);
    if (st.in(&a.y, 0, reduced->x, N * nr) || st.in(&a.lamr, 1, reduced->lam, N * mr) || st.in(&a.fvalr, 2, reduced->fval, N) ||
        st.in(&a.softr, 3, reduced->soft_slack, N) || st.in(&a.flagr, 4, reduced->exitflag, N) || st.in(&a.iterr, 5, reduced->iter, N) ||
        st.out(&a.x, 6, full->x, N * n) || st.out(&a.lam, 7, full->lam, N * m) || st.out(&a.fval, 8, full->fval, N) ||
        st.out(&a.soft, 9, full->soft_slack, N) || st.out(&a.exitflag, 10, full->exitflag, N) || st.out(&a.iter, 11, full->iter, N))
        return DAQP_EXIT_UNSUPPORTED;
    void (*k)(ElimDev, ExpandArgs) = elim_pick(d.n, k_expand<1>, k_expand<2>, k_expand<4>, k_expand<8>);
    hipLaunchKernelGGL(k, dim3(d.N), dim3(64), 0, el->stream, d, a);
    HIPCHK(hipGetLastError());
    return st.finish();
}

int daqp_batch_elimination_basis(DAQPBatchElimination *el, c_float *x0, c_float *Z, c_float *c0, int memory)
{
    int ndev = 0;
    if (elim_no_device(&ndev)) return DAQP_EXIT_UNSUPPORTED;
    if (!el) { set_err("daqp_batch_elimination_basis: null handle"); return DAQP_EXIT_UNSUPPORTED; }
    if (memory != DAQP_MEM_HOST && memory != DAQP_MEM_DEVICE) { set_err("daqp_batch_elimination_basis: memory must be DAQP_MEM_HOST or DAQP_MEM_DEVICE"); return DAQP_EXIT_UNSUPPORTED; }
    HIPCHK(hipSetDevice(el->device));
    const ElimDev &d = el->d;
    const size_t N = d.N, n = d.n, nr = d.nr;
    const hipMemcpyKind kind = memory == DAQP_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (x0) HIPCHK(hipMemcpyAsync(x0, d.x0, sizeof(double) * N * n, kind, el->stream));
    if (c0) HIPCHK(hipMemcpyAsync(c0, d.c0, sizeof(double) * N, kind, el->stream));
    Staging st(nullptr, nullptr, el->stream, memory);
    double *Zd = nullptr;
    if (st.out(&Zd, 0, Z, N * n * nr)) return DAQP_EXIT_UNSUPPORTED;
    if (Zd) {
        void (*k)(ElimDev, double *) = elim_pick(d.n, k_elim_basis<1>, k_elim_basis<2>, k_elim_basis<4>, k_elim_basis<8>);
        hipLaunchKernelGGL(k, dim3(d.N), dim3(64), 0, el->stream, d, Zd);
        HIPCHK(hipGetLastError());
    }
    if (memory == DAQP_MEM_HOST) HIPCHK(hipStreamSynchronize(el->stream));
    return st.finish();
}

int daqp_batch_elimination_read(DAQPBatchElimination *el, c_float *H, c_float *f, c_float *A, c_float *bupper, c_float *blower, int *sense, int memory)
{
    int ndev = 0;
    if (elim_no_device(&ndev)) return DAQP_EXIT_UNSUPPORTED;
    if (!el) { set_err("daqp_batch_elimination_read: null handle"); return DAQP_EXIT_UNSUPPORTED; }
    if (memory != DAQP_MEM_HOST && memory != DAQP_MEM_DEVICE) { set_err("daqp_batch_elimination_read: memory must be DAQP_MEM_HOST or DAQP_MEM_DEVICE"); return DAQP_EXIT_UNSUPPORTED; }
    const ElimDev &d = el->d;
    if (H && d.lp) { set_err("daqp_batch_elimination_read: an LP batch has no reduced H"); return DAQP_EXIT_UNSUPPORTED; }
    HIPCHK(hipSetDevice(el->device));
    const size_t N = d.N, nr = d.nr, mr = d.mr;
    const hipMemcpyKind kind = memory == DAQP_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (H) HIPCHK(hipMemcpyAsync(H, d.Hr, sizeof(double) * N * nr * nr, kind, el->stream));
    if (f) HIPCHK(hipMemcpyAsync(f, d.fr, sizeof(double) * N * nr, kind, el->stream));
    if (A && mr) HIPCHK(hipMemcpyAsync(A, d.Ar, sizeof(double) * N * mr * nr, kind, el->stream));
    if (bupper && mr) HIPCHK(hipMemcpyAsync(bupper, d.bur, sizeof(double) * N * mr, kind, el->stream));
    if (blower && mr) HIPCHK(hipMemcpyAsync(blower, d.blr, sizeof(double) * N * mr, kind, el->stream));
    if (sense && mr) HIPCHK(hipMemcpyAsync(sense, d.senser, sizeof(int) * N * mr, kind, el->stream));
    if (memory == DAQP_MEM_HOST) HIPCHK(hipStreamSynchronize(el->stream));
    return 0;
}

// The adjoint of an eliminated batch (include/daqp_amd.h, eliminate_adjoint.hip.h): reduce the right-hand side, the adjoint of the
// reduced batch (backward_launch on the handle's device buffers: it only enqueues), expand -- three launches on the handle's stream
// (four where `which` == 0 adds the null-space kernel).  Every refusal, backward_launch's own included, comes before the first launch.
int daqp_batch_eliminate_backward(DAQPBatchElimination *el, DAQPBatch *reduced, const c_float *grad_x, const c_float *grad_lam,
                                  c_float *dz, c_float *dbupper, c_float *dblower, int *status, int which, int memory)
{
    const char *who = "daqp_batch_eliminate_backward";
    int ndev = 0;
    if (elim_no_device(&ndev)) return DAQP_EXIT_UNSUPPORTED;
    if (!el || !reduced || !dz || !dbupper || !dblower || !status) { set_err("%s: null handle, batch or output array", who); return DAQP_EXIT_UNSUPPORTED; }
    if (!grad_x && !grad_lam) { set_err("%s: grad_x and grad_lam are both null: there is nothing to differentiate", who); return DAQP_EXIT_UNSUPPORTED; }
    if (which < -1 || which > 1) { set_err("%s: which must be -1 (Gram only), 0 (null space for the proximal problems) or 1 (null space for every problem)", who); return DAQP_EXIT_UNSUPPORTED; }
    if (memory != DAQP_MEM_HOST && memory != DAQP_MEM_DEVICE) { set_err("%s: memory must be DAQP_MEM_HOST or DAQP_MEM_DEVICE", who); return DAQP_EXIT_UNSUPPORTED; }
    const ElimDev &d = el->d;
    const BatchDev &rb = reduced->d;
    if (rb.N != d.N || rb.n != d.nr || rb.m != d.mr || rb.ms != 0) {
        set_err("%s: the reduced batch has shape (N, n, m, ms) = (%d, %d, %d, %d), the handle's reduced problem (%d, %d, %d, 0)", who, rb.N, rb.n, rb.m, rb.ms, d.N, d.nr, d.mr);
        return DAQP_EXIT_UNSUPPORTED;
    }
    if (reduced->device != el->device) { set_err("%s: the reduced batch is on device %d, the handle on device %d", who, reduced->device, el->device); return DAQP_EXIT_UNSUPPORTED; }
    if (reduced->stream != el->stream) { set_err("%s: the reduced batch and the handle are on different streams: the three launches are ordered by sharing one", who); return DAQP_EXIT_UNSUPPORTED; }
    if (reduced->plan.ns_max > 0) { set_err("%s: reduced batches created with ns_max > 0 (soft constraints) are not supported: a SOFT kept row is weighted by the reduced q_k", who); return DAQP_EXIT_UNSUPPORTED; }
    if (which == 1 && d.nr > 64) { set_err("%s: which == 1 needs nr <= 64 (nr = %d): the null-space kernel holds a problem in one wavefront", who, d.nr); return DAQP_EXIT_UNSUPPORTED; }
    if (!reduced->is_setup || !reduced->solved || reduced->pending_mask) {
        set_err("%s: the last operation on the reduced batch was not a successful daqp_batch_solve", who);
        return DAQP_EXIT_UNSUPPORTED;
    }
    if (which >= 0 && rb.H == nullptr) { set_err("%s: the reduced batch has no Hessian of the handle's to read", who); return DAQP_EXIT_UNSUPPORTED; }
    if (which != 1 && !pick_tier(rb.n, rb.cap, backward_lds_bytes).fits) { set_err("%s: nr = %d with working sets of %d rows does not fit the adjoint kernel", who, rb.n, rb.cap); return DAQP_EXIT_UNSUPPORTED; }
    HIPCHK(hipSetDevice(el->device));
    const size_t N = d.N, n = d.n, m = d.m, nr = d.nr, mr = d.mr;
    if (!el->adj_str) {
        if (elim_alloc(el, &el->adj_gy, N * nr) || elim_alloc(el, &el->adj_glr, N * mr) || elim_alloc(el, &el->adj_dz0, N * n) ||
            elim_alloc(el, &el->adj_dzr, N * nr) || elim_alloc(el, &el->adj_dbur, N * mr) || elim_alloc(el, &el->adj_dblr, N * mr) ||
            elim_alloc(el, &el->adj_str, N))
            return DAQP_EXIT_UNSUPPORTED;
    }
    ElimAdjointArgs a{};
    a.grad_y = el->adj_gy; a.grad_lam_r = el->adj_glr; a.dz0 = el->adj_dz0;
    a.dz_r = el->adj_dzr; a.dbu_r = el->adj_dbur; a.dbl_r = el->adj_dblr; a.status_r = el->adj_str;
    Staging st(nullptr, nullptr, el->stream, memory);
    if (st.in(&a.grad_x, 0, grad_x, N * n) || st.in(&a.grad_lam, 1, grad_lam, N * m) || st.out(&a.dz, 2, dz, N * n) ||
        st.out(&a.dbupper, 3, dbupper, N * m) || st.out(&a.dblower, 4, dblower, N * m) || st.out(&a.status, 5, status, N))
        return DAQP_EXIT_UNSUPPORTED;
    void (*kr)(ElimDev, ElimAdjointArgs) = elim_pick(d.n, k_adjoint_reduce<1>, k_adjoint_reduce<2>, k_adjoint_reduce<4>, k_adjoint_reduce<8>);
    hipLaunchKernelGGL(kr, dim3(d.N), dim3(64), 0, el->stream, d, a);
    HIPCHK(hipGetLastError());
    if (backward_launch(who, reduced, a.grad_y, a.dz_r, a.dbu_r, a.dbl_r, nullptr, nullptr, nullptr, a.status_r, DAQP_MEM_DEVICE, which,
                        grad_lam ? a.grad_lam_r : nullptr))
        return DAQP_EXIT_UNSUPPORTED;
    void (*ke)(ElimDev, ElimAdjointArgs) = elim_pick(d.n, k_adjoint_expand<1>, k_adjoint_expand<2>, k_adjoint_expand<4>, k_adjoint_expand<8>);
    hipLaunchKernelGGL(ke, dim3(d.N), dim3(64), 0, el->stream, d, a);
    HIPCHK(hipGetLastError());
    return st.finish();
}

unsigned long long daqp_batch_elimination_bytes(const DAQPBatchElimination *el) { return el ? el->bytes : 0; }

void daqp_batch_elimination_free(DAQPBatchElimination *el)
{
    if (!el) return;
    (void)hipSetDevice(el->device);
    (void)hipStreamSynchronize(el->stream);
    for (void *p : el->owned) (void)hipFree(p);
    delete el;
}

int daqp_batch_backward(DAQPBatch *b, const c_float *grad_x, c_float *dz, c_float *dbupper, c_float *dblower, int *status, int memory)
{
    if (!b || !grad_x || !dz || !dbupper || !dblower || !status) { set_err("daqp_batch_backward: null batch or array"); return DAQP_EXIT_UNSUPPORTED; }
    if (b->plan.ns_max > 0) { set_err("daqp_batch_backward: batches created with ns_max > 0 (soft constraints) are not supported: daqp_batch_backward_soft"); return DAQP_EXIT_UNSUPPORTED; }
    return backward_launch("daqp_batch_backward", b, grad_x, dz, dbupper, dblower, nullptr, nullptr, nullptr, status, memory);
}

// The adjoint without a factor of H (nullspace.hip.h): which == 0 -- daqp_batch_backward, then the null-space kernel for the problems
// that went through the proximal loop; which == 1 -- the null-space kernel for every problem.  It reads the caller's H and A in place.
int daqp_batch_backward_nullspace(DAQPBatch *b, const c_float *grad_x, c_float *dz, c_float *dbupper, c_float *dblower, int *status, int which, int memory)
{
    if (!b || !grad_x || !dz || !dbupper || !dblower || !status) { set_err("daqp_batch_backward_nullspace: null batch or array"); return DAQP_EXIT_UNSUPPORTED; }
    if (b->plan.ns_max > 0) { set_err("daqp_batch_backward_nullspace: batches created with ns_max > 0 (soft constraints) are not supported: q_k = c_k H^-1 c_k' does not exist for a singular H"); return DAQP_EXIT_UNSUPPORTED; }
    if (which != 0 && which != 1) { set_err("daqp_batch_backward_nullspace: which must be 0 (proximal problems only) or 1 (every problem)"); return DAQP_EXIT_UNSUPPORTED; }
    if (which == 1 && b->d.n > 64) { set_err("daqp_batch_backward_nullspace: which == 1 needs n <= 64 (n = %d): the null-space kernel holds a problem in one wavefront", b->d.n); return DAQP_EXIT_UNSUPPORTED; }
    if (b->is_setup && b->d.H == nullptr) { set_err("daqp_batch_backward_nullspace: the batch has no Hessian of the caller's to read"); return DAQP_EXIT_UNSUPPORTED; }
    return backward_launch("daqp_batch_backward_nullspace", b, grad_x, dz, dbupper, dblower, nullptr, nullptr, nullptr, status, memory, which);
}

// The same for batches with soft rows (and, with identical results, for batches without): q_k, u_k and the ids of the SOFT rows of
// each working set come back with the adjoint.  A batch with ns_max == 0 has none: its qsoft is zero, usoft / usoft_id are empty.
int daqp_batch_backward_soft(DAQPBatch *b, const c_float *grad_x, c_float *dz, c_float *dbupper, c_float *dblower,
                             c_float *qsoft, c_float *usoft, int *usoft_id, int *status, int memory)
{
    if (!b || !grad_x || !dz || !dbupper || !dblower || !status) { set_err("daqp_batch_backward_soft: null batch or array"); return DAQP_EXIT_UNSUPPORTED; }
    const int rc = backward_launch("daqp_batch_backward_soft", b, grad_x, dz, dbupper, dblower, qsoft, usoft, usoft_id, status, memory);
    if (rc == 0 && b->plan.ns_max == 0 && qsoft && b->d.m) {      // no SOFT instantiation ran: no row of any working set is soft
        const size_t bytes = sizeof(double) * (size_t)b->d.N * b->d.m;
        if (memory == DAQP_MEM_DEVICE) HIPCHK(hipMemsetAsync(qsoft, 0, bytes, b->stream));
        else memset(qsoft, 0, bytes);
    }
    return rc;
}

// The adjoint with a dual right-hand side (include/daqp_amd.h): K [dz; dnu] = [grad_x; grad_lam on W].  grad_lam == NULL is the
// existing entry for the same `which`, kernels and all; otherwise the DUAL instantiations run in the same places.
int daqp_batch_backward_dual(DAQPBatch *b, const c_float *grad_x, const c_float *grad_lam, c_float *dz, c_float *dbupper, c_float *dblower,
                             int *status, int which, int memory)
{
    if (!b || !dz || !dbupper || !dblower || !status) { set_err("daqp_batch_backward_dual: null batch or output array"); return DAQP_EXIT_UNSUPPORTED; }
    if (!grad_x && !grad_lam) { set_err("daqp_batch_backward_dual: grad_x and grad_lam are both null: there is nothing to differentiate"); return DAQP_EXIT_UNSUPPORTED; }
    if (which < -1 || which > 1) { set_err("daqp_batch_backward_dual: which must be -1 (Gram only), 0 (null space for the proximal problems) or 1 (null space for every problem)"); return DAQP_EXIT_UNSUPPORTED; }
    if (b->plan.ns_max > 0) { set_err("daqp_batch_backward_dual: batches created with ns_max > 0 (soft constraints) are not supported: the multiplier of a soft row is not built here"); return DAQP_EXIT_UNSUPPORTED; }
    if (which == 1 && b->d.n > 64) { set_err("daqp_batch_backward_dual: which == 1 needs n <= 64 (n = %d): the null-space kernel holds a problem in one wavefront", b->d.n); return DAQP_EXIT_UNSUPPORTED; }
    if (which >= 0 && b->is_setup && b->d.H == nullptr) { set_err("daqp_batch_backward_dual: the batch has no Hessian of the caller's to read"); return DAQP_EXIT_UNSUPPORTED; }
    if (!grad_lam) return which < 0 ? daqp_batch_backward(b, grad_x, dz, dbupper, dblower, status, memory)
                                    : daqp_batch_backward_nullspace(b, grad_x, dz, dbupper, dblower, status, which, memory);
    return backward_launch("daqp_batch_backward_dual", b, grad_x, dz, dbupper, dblower, nullptr, nullptr, nullptr, status, memory, which, grad_lam);
}

// The adjoint of a batch with soft rows with a dual right-hand side (include/daqp_amd.h): K [dz; dnu] = [grad_x; ghat_lam on W], K with -S
// in its (2,2) block.  No dual gradient is daqp_batch_backward_soft itself; a batch without soft rows has no S and no soft_slack, so
// grad_slack meets no row there and the call is daqp_batch_backward_dual(which = -1), kernels and all, then the zeroed qsoft.
int daqp_batch_backward_soft_dual(DAQPBatch *b, const c_float *grad_x, const c_float *grad_lam, const c_float *grad_slack, const c_float *lam,
                                  c_float *dz, c_float *dbupper, c_float *dblower, c_float *qsoft, c_float *usoft, int *usoft_id,
                                  int *status, int memory)
{
    const char *who = "daqp_batch_backward_soft_dual";
    if (!b || !dz || !dbupper || !dblower || !status) { set_err("%s: null batch or output array", who); return DAQP_EXIT_UNSUPPORTED; }
    if (!grad_x && !grad_lam && !grad_slack) { set_err("%s: grad_x, grad_lam and grad_slack are all null: there is nothing to differentiate", who); return DAQP_EXIT_UNSUPPORTED; }
    if (grad_slack && !lam) { set_err("%s: grad_slack needs lam, the multipliers of the solve (null)", who); return DAQP_EXIT_UNSUPPORTED; }
    if (!grad_lam && !grad_slack) return daqp_batch_backward_soft(b, grad_x, dz, dbupper, dblower, qsoft, usoft, usoft_id, status, memory);
    int rc;
    if (b->plan.ns_max == 0) {
        if (!grad_x && !grad_lam) { set_err("%s: grad_slack alone on a batch created with ns_max == 0: it has no soft row, there is nothing to differentiate", who); return DAQP_EXIT_UNSUPPORTED; }
        rc = daqp_batch_backward_dual(b, grad_x, grad_lam, dz, dbupper, dblower, status, -1, memory);
        if (rc == 0 && qsoft && b->d.m) {      // no SOFT instantiation ran: no row of any working set is soft
            const size_t bytes = sizeof(double) * (size_t)b->d.N * b->d.m;
            if (memory == DAQP_MEM_DEVICE) HIPCHK(hipMemsetAsync(qsoft, 0, bytes, b->stream));
            else memset(qsoft, 0, bytes);
        }
        return rc;
    }
    return backward_launch(who, b, grad_x, dz, dbupper, dblower, qsoft, usoft, usoft_id, status, memory, -1, grad_lam, true, grad_slack, lam);
}

// Iterative refinement of (x, lam) at the stored working set (include/daqp_amd.h): refine_launch above
int daqp_batch_refine(DAQPBatch *b, c_float *x, c_float *lam, c_float *fval, c_float *residual, int *steps, int *status, int max_steps, int memory)
{
    return refine_launch("daqp_batch_refine", b, x, lam, fval, residual, steps, status, max_steps, memory);
}

// The refinement without a factor of H (refine_nullspace.hip.h): which == 0 -- daqp_batch_refine, then the null-space kernel for the
// problems that went through the proximal loop; which == 1 -- the null-space kernel for every problem.  It reads the caller's H, f, A
// and bounds in place.
int daqp_batch_refine_nullspace(DAQPBatch *b, c_float *x, c_float *lam, c_float *fval, c_float *residual, int *steps, int *status,
                                int max_steps, int which, int memory)
{
    if (which != 0 && which != 1) { set_err("daqp_batch_refine_nullspace: which must be 0 (proximal problems only) or 1 (every problem)"); return DAQP_EXIT_UNSUPPORTED; }
    return refine_launch("daqp_batch_refine_nullspace", b, x, lam, fval, residual, steps, status, max_steps, memory, which);
}

// daqp_certify_batch (include/daqp_amd.h, certify.hip.h): residuals and ray measures of (x, lam), stateless
int daqp_certify_batch(DAQPBatchCertificate *out, const DAQPBatchProblem *p, const c_float *x, const c_float *lam, int shared, int device, void *hip_stream)
{
    if (!out || !p || !x || !lam) { set_err("daqp_certify_batch: null out, problem, x or lam"); return DAQP_EXIT_UNSUPPORTED; }
    if (p->N <= 0 || p->n <= 0 || p->n > 511 || p->m < 0 || p->m > (1 << 24) || p->ms < 0 || p->ms > p->n || p->ms > p->m) {
        set_err("daqp_certify_batch: bad dimensions N=%d n=%d m=%d ms=%d (N >= 1, 1 <= n <= 511, 0 <= m <= 2^24, ms <= n, ms <= m)", p->N, p->n, p->m, p->ms);
        return DAQP_EXIT_UNSUPPORTED;
    }
    if (!p->f || (p->m > p->ms && !p->A) || (p->m > 0 && (!p->bupper || !p->blower))) {
        set_err("daqp_certify_batch: null f, A or bounds");
        return DAQP_EXIT_UNSUPPORTED;
    }
    if (p->memory != DAQP_MEM_HOST && p->memory != DAQP_MEM_DEVICE) { set_err("daqp_certify_batch: memory must be DAQP_MEM_HOST or DAQP_MEM_DEVICE"); return DAQP_EXIT_UNSUPPORTED; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        set_err("no HIP device: libdaqp_amd has no CPU path");
        return DAQP_EXIT_UNSUPPORTED;
    }
    if (device < 0) { if (hipGetDevice(&device) != hipSuccess) device = 0; }
    if (device >= ndev) { set_err("daqp_certify_batch: device %d of %d", device, ndev); return DAQP_EXIT_UNSUPPORTED; }
    HIPCHK(hipSetDevice(device));
    if (device < 64) g_devices_used.fetch_or(1ull << device);
    return certify_run(out, p, x, lam, shared, reinterpret_cast<hipStream_t>(hip_stream));
}

} // extern "C"
