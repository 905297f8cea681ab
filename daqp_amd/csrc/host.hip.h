// daqp_amd/csrc/host.hip.h -- what the host translation units of libdaqp_amd.so share: the batch object, the error text and the device
// allocator.  daqp_amd.hip defines what is only declared here; none of it is an exported symbol of the library.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <memory>
#include <string>
#include <vector>

#include "batch_dev.hip.h"
#include "plan.hip.h"

#define DAQP_INTERNAL __attribute__((visibility("hidden")))
namespace daqp_amd {
struct ProxDev;      // prox.hip.h (which defines kernels, so only daqp_amd.hip includes it)
DAQP_INTERNAL void set_err(const char *fmt, ...);      // the text behind daqp_amd_last_error(): one thread-local buffer
#define HIPCHK(expr)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            set_err("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return DAQP_EXIT_UNSUPPORTED;                                                     \
        }                                                                                     \
    } while (0)
DAQP_INTERNAL extern std::atomic<unsigned long long> g_devices_used;   // bit per device that some call has set: daqp_amd_shutdown
// what one family of post-solve calls (post_solve.hip) keeps on the batch: one each, so that a call of one leaves the other's as it is
struct PostSolveBufs {
    double *scratch = nullptr; int grid = 0;   // [grid][the kernel's *_scratch_doubles]: rows and Gram matrix of shapes that LDS does not hold
    void *slot[11] = {};        // device copies of host-resident arguments, in the order the entry stages them (each allocated when first needed)
};
} // namespace daqp_amd

struct DAQPBatch {
    DAQP_INTERNAL DAQPBatch();
    int device = 0;
    hipStream_t stream = nullptr;
    daqp_amd::BatchDev d{};
    std::vector<void *> owned;
    unsigned long long bytes = 0;
    // staging copies of host inputs (allocated on first use)
    double *sH = nullptr, *sf = nullptr, *sA = nullptr, *sbu = nullptr, *sbl = nullptr;
    int *ssense = nullptr;
    size_t nH = 0, nf = 0, nA = 0, nbu = 0, nbl = 0, nsense = 0;   // elements each staging slot can hold
    bool was_shared = false;   // last set up by daqp_batch_setup_shared: d.H / d.A are ONE matrix, not N
    // library-owned result buffers
    double *ox = nullptr, *olam = nullptr, *ofval = nullptr, *osoft = nullptr;
    int *oflag = nullptr, *oiter = nullptr;
    DAQPSettings *st_dev = nullptr;
    daqp_amd::BatchDev *d_dev = nullptr;
    daqp_amd::SolvePlan plan;   // how this shape is solved (plan.hip.h): written by batch_create, read by everything else
    double *fact_buf = nullptr;     // [N][4] records of k_fact_wg (setup_fact.hip.h), allocated for the shapes it serves
    bool in_prox_loop = false;      // launches of the proximal outer loop (solve_with_prox)
    // hand-overs of the last solve launch, counted on the device and copied to pinned memory without waiting: when most of a batch goes to the
    // full-register kernel anyway (working sets beyond what the image kernel holds), the next launches go there directly; every 16th tries again
    int *img_ho_pin = nullptr;
    unsigned img_skipped = 0;
    double *wide_u = nullptr, *wide_l = nullptr;   // daqp_batch_setup_shared: +-1e30 bounds of the one factorisation
    int *structural = nullptr, *shared_flag = nullptr;
    bool exact_sticky = false;   // the sense of some working-set rows was replaced without the working set being rebuilt (a sense update without a
                                 // sense array, utils.c:85-86; an update that took the new sense and then failed its bound check, utils.c:88-96): the
                                 // reference iterates on from that state, and only its own arithmetic does the same (the default mode's carried
                                 // intermediate results assume the flags they were formed with) -- solves use the exact kernels until the next update
    int part_mask = 0;      // the last (re-)setup was a partial daqp_batch_update with this mask (k_setup<..., PART>): its regularising re-runs use the same kernel
    int pending_mask = 0;   // daqp_batch_update(UPDATE_v|UPDATE_d) not yet applied: the next solve launch does it (k_ldp_reg mode 2)
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool timed_setup = false, timed_solve = false;
    bool is_setup = false;
    // proximal outer loop (prox.hip.h): buffers appear with the first singular Hessian
    std::unique_ptr<daqp_amd::ProxDev, void (*)(daqp_amd::ProxDev *)> px_own;   // (the type is complete in daqp_amd.hip only, whose constructor makes it)
    daqp_amd::ProxDev &px;
    bool prox_ready = false;
    int counter_host[4] = {0, 0, 0, 0};   // read-back of px.counter
    // "is any Hessian singular?" after a setup: counted on the device, copied to pinned memory without waiting.  The next solve
    // goes out FIRST (flagged problems sit it out), then the host looks at the count: no gap between the setup and the solve
    // launch on the device.  Anything else that needs the final setup flags resolves the question first (resolve_setup).
    int *pin_count = nullptr;
    hipEvent_t ev_count = nullptr;
    bool reg_pending = false;
    int reg_mask = 0;
    int n_prox_qps = 0;            // problems of the current setup that go through the outer loop
    int prox_outer = 0;            // outer iterations of the last solve (the longest loop of the batch)
    double *ident = nullptr;       // LP batches (H == NULL): the one n x n identity the setup pass reads as H
    // single-problem workspaces: results of the last daqp_ldp, waiting for daqp_extract_result
    // single-problem batches (N == 1, the daqp_quadprog / setup_daqp path): one pinned host slab and one device slab each for
    // the inputs and the results (one copy each way instead of six), and the pool key of a parked batch
    char *pin_in = nullptr, *dev_in = nullptr, *pin_out = nullptr;
    size_t in_cap = 0, out_bytes = 0;
    double *dev_mir = nullptr, *pin_mir = nullptr;   // host mirrors of a single-problem workspace: gathered slab (k_mirror) and its pinned landing zone
    // One problem, latency: the result slab and the mirror slab are MAPPED host memory that the kernels write themselves, and the host
    // learns that they are there from a mapped word written by a one-thread kernel at the end of the stream's work -- no hipMemcpy, no
    // stream synchronisation on the way of daqp_quadprog / daqp_solve / daqp_update_ldp (0.34 / 0.14 ms per call were
    // launches, small copies and synchronisations around ~0.1 ms / ~0.02 ms of kernels)
    daqp_amd::BatchDev d_pushed{};        // what d_dev holds (the register kernels read the descriptor through it): pushed again only when it differs
    bool pushed_valid = false;
    bool mapped_out = false, mapped_mir = false;     // ox .. oiter / dev_mir point into pin_out / pin_mir through their device addresses
    int *pin_sig = nullptr, *pin_sig_dev = nullptr;  // the completion word and its device address
    int sig_seq = 0;
    bool lean = false;          // daqp_quadprog: no count of flagged Hessians, no activation launch (the solve launch activates; a flagged problem comes back with the internal code and takes the full path)
    bool defer_wait = false;    // daqp_batch_solve only enqueues: the caller puts more work behind it, waits once and collects (daqp_ldp)
    bool recheck_due = false;   // one problem: the second pass of an INFEASIBLE verdict is decided after the wait, on the host
    char *pin_upd = nullptr, *pin_upd_dev = nullptr;  // f / bupper / blower of a deferred daqp_update_ldp(v|d): mapped, read by the solve launch in place
    bool mirror_ldp_due = false;   // a deferred update's v / d have not reached the host mirrors yet: the next solve's gather brings them
    hipEvent_t ev_in = nullptr;     // the last packed host->device copy (the pinned slab is free again once it has run)
    std::string env_key;
    int dev_cus = 0, dev_per_cu = 0, dev_tier_attr_ok = 0, dev_per_cu_tier = 0;   // what batch_create asked of the device for the plan (0: not asked)
    unsigned long long *tstart = nullptr;   // [N] start stamps of the current daqp_batch_solve (allocated when a time limit is first armed)
    std::vector<double> one_lam;
    double one_fval = 0, one_soft = 0;
    int one_flag = 0, one_iter = 0;
    bool one_valid = false;   // one_* belong to the workspace's current LDP (cleared by setup / update / a failed solve)
    // default arithmetic: INFEASIBLE verdicts of a solve straight after a setup are re-derived in the reference's arithmetic (recheck.hip.h)
    bool fresh = false;        // the state is that of the last daqp_batch_setup (own H / A per problem, not an LP): nothing solved or updated since
    int fresh_mask = 0;        // its init_mask
    bool recheck = true;       // DAQP_AMD_NO_RECHECK=1 switches the second pass off
    int recheck_device = -1;   // the same for inputs that were ADOPTED (DAQP_MEM_DEVICE: the second pass reads them again at solve time): -1 = not said
                               // (on, unless DAQP_AMD_RECHECK_DEVICE=0), 0 / 1 = daqp_batch_set_recheck
    bool inputs_adopted = false;   // the last setup's inputs were device arrays of the caller's, used in place
    bool quiet_setup = false;  // the setup that runs now is the second pass of a one-problem batch: the caller's setup events stay as they are
    hipEvent_t ev_r[2] = {nullptr, nullptr};   // around the second pass (daqp_batch_recheck_ms)
    bool timed_recheck = false;
    DAQPBatch *redo = nullptr; // companion batch in the exact mode (created with the first infeasible verdict, grown on demand)
    int *redo_list = nullptr, *redo_count = nullptr, *pin_redo = nullptr, *pin_redo_dev = nullptr;   // pin_redo: a mapped host word the marking kernel writes
    int rechecked = 0;         // problems the last solve sent through the second pass
    // the post-solve calls (post_solve.hip)
    bool solved = false;       // the last operation on the batch was a successful daqp_batch_solve: the stored iterate is that of the reported optimum
    daqp_amd::PostSolveBufs adjoint;   // daqp_batch_backward* (backward.hip.h, nullspace.hip.h)
    daqp_amd::PostSolveBufs refine;    // daqp_batch_refine (refine.hip.h)
};

namespace daqp_amd {
template <typename T>
DAQP_INTERNAL int dev_alloc(DAQPBatch *b, T **p, size_t count)
{
    if (count == 0) count = 1;
    HIPCHK(hipMalloc(reinterpret_cast<void **>(p), count * sizeof(T)));
    b->owned.push_back(*p);
    b->bytes += count * sizeof(T);
    return 0;
}
} // namespace daqp_amd
