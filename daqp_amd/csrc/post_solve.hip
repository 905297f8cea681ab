// post_solve.hip -- host side of the calls that run behind a solve: the adjoint (daqp_batch_backward*), the refinement
// (daqp_batch_refine, daqp_batch_refine_nullspace) and the certificate (daqp_certify_batch).  Each is argument checks, one or two
// launches and the three helpers below; the kernels are in backward_kernel.hip, refine_kernel.hip and certify_kernel.hip.
#include <cstring>

#include "host.hip.h"
#include "backward.hip.h"
#include "nullspace.hip.h"
#include "certify.hip.h"
#include "refine.hip.h"
#include "refine_nullspace.hip.h"

namespace daqp_amd {
// the adjoint kernel: backward_kernel.hip
extern template __global__ void k_backward<64, true, true, false>(BatchDev, BackwardArgs);
extern template __global__ void k_backward<256, false, true, false>(BatchDev, BackwardArgs);
extern template __global__ void k_backward<256, false, false, false>(BatchDev, BackwardArgs);
extern template __global__ void k_backward<64, true, true, true>(BatchDev, BackwardArgs);
extern template __global__ void k_backward<256, false, true, true>(BatchDev, BackwardArgs);
extern template __global__ void k_backward<256, false, false, true>(BatchDev, BackwardArgs);
extern template __global__ void k_backward_nullspace<64>(BatchDev, NullspaceArgs);
}

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
int backward_launch(const char *who, DAQPBatch *b, const c_float *grad_x, c_float *dz, c_float *dbupper, c_float *dblower,
                    c_float *qsoft, c_float *usoft, int *usoft_id, int *status, int memory, int nsw = -1)
{
    if (!b->is_setup || !b->solved || b->pending_mask) {
        set_err("%s: the last operation on the batch was not a successful daqp_batch_solve", who);
        return DAQP_EXIT_UNSUPPORTED;
    }
    HIPCHK(hipSetDevice(b->device));
    const BatchDev &d = b->d;
    const size_t N = d.N, n = d.n, m = d.m, ns = b->ns_max;
    const bool soft = b->ns_max > 0;
    if (!soft) qsoft = nullptr, usoft = nullptr, usoft_id = nullptr;      // (ns_max == 0: usoft / usoft_id are empty, qsoft is zeroed by the entry)
    const Tier t = pick_tier(d.n, d.cap, backward_lds_bytes);
    if (!t.fits && nsw != 1) { set_err("%s: n = %d with working sets of %d rows does not fit the adjoint kernel", who, d.n, d.cap); return DAQP_EXIT_UNSUPPORTED; }
    void (*kb)(BatchDev, BackwardArgs);
    if (soft) kb = t.small ? k_backward<64, true, true, true> : (t.nl ? k_backward<256, false, true, true> : k_backward<256, false, false, true>);
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
        st.out(&a.usoft_id, 6, usoft_id, N * ns) || st.out(&a.status, 7, status, N))
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
        const size_t lds_ns = nullspace_lds_bytes(d.n);
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_backward_nullspace<64>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_ns));
        hipLaunchKernelGGL(k_backward_nullspace<64>, dim3(d.N), dim3(64), lds_ns, b->stream, d, na);
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
    if (b->ns_max > 0) { set_err("%s: batches created with ns_max > 0 (soft constraints) are not supported: soft rows change the (2,2) block of the system", who); return DAQP_EXIT_UNSUPPORTED; }
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

} // namespace

extern "C" {

int daqp_batch_backward(DAQPBatch *b, const c_float *grad_x, c_float *dz, c_float *dbupper, c_float *dblower, int *status, int memory)
{
    if (!b || !grad_x || !dz || !dbupper || !dblower || !status) { set_err("daqp_batch_backward: null batch or array"); return DAQP_EXIT_UNSUPPORTED; }
    if (b->ns_max > 0) { set_err("daqp_batch_backward: batches created with ns_max > 0 (soft constraints) are not supported: daqp_batch_backward_soft"); return DAQP_EXIT_UNSUPPORTED; }
    return backward_launch("daqp_batch_backward", b, grad_x, dz, dbupper, dblower, nullptr, nullptr, nullptr, status, memory);
}

// The adjoint without a factor of H (nullspace.hip.h): which == 0 -- daqp_batch_backward, then the null-space kernel for the problems
// that went through the proximal loop; which == 1 -- the null-space kernel for every problem.  It reads the caller's H and A in place.
int daqp_batch_backward_nullspace(DAQPBatch *b, const c_float *grad_x, c_float *dz, c_float *dbupper, c_float *dblower, int *status, int which, int memory)
{
    if (!b || !grad_x || !dz || !dbupper || !dblower || !status) { set_err("daqp_batch_backward_nullspace: null batch or array"); return DAQP_EXIT_UNSUPPORTED; }
    if (b->ns_max > 0) { set_err("daqp_batch_backward_nullspace: batches created with ns_max > 0 (soft constraints) are not supported: q_k = c_k H^-1 c_k' does not exist for a singular H"); return DAQP_EXIT_UNSUPPORTED; }
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
    if (rc == 0 && b->ns_max == 0 && qsoft && b->d.m) {      // no SOFT instantiation ran: no row of any working set is soft
        const size_t bytes = sizeof(double) * (size_t)b->d.N * b->d.m;
        if (memory == DAQP_MEM_DEVICE) HIPCHK(hipMemsetAsync(qsoft, 0, bytes, b->stream));
        else memset(qsoft, 0, bytes);
    }
    return rc;
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
