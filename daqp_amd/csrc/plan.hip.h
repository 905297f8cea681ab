// daqp_amd/csrc/plan.hip.h -- how a batch shape is solved, decided in ONE place and on the host alone: the DAQP_AMD_* switches (Tuning), the
// kernel family / register shape / fp32 image / workgroup kernel / setup kernel / LDS sizes / scratch buffers of a shape (SolvePlan: plan_shape,
// then plan_device with three numbers asked of the device), the launch sequence of a solve (pick_path) and the kernel tables behind them.
// Nothing here calls the HIP runtime: it is arithmetic on (N, n, m, ms, ns_max), the switches and the layout functions of the kernel headers, so
// it runs -- and is tested (tests/test_cpu_plan.py, daqp_amd_describe_plan) -- without a device.  batch_create (daqp_amd.hip) asks the device,
// allocates what the plan names and copies the plan's share of the descriptor (plan_fill); after that the plan is read only.
#pragma once
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "batch_dev.hip.h"
#include "wg_layout.hip.h"
#ifndef DAQP_AMD_PLAN_TYPES_ONLY   // (a unit that only reads plans -- post_solve.hip -- stays clear of the kernel headers, which define kernels)
#include "kernels.hip.h"
#include "reg_kernel.hip.h"
#include "setup_fast.hip.h"
#include "setup_fact.hip.h"
#include "tiny_setup.hip.h"
#endif

namespace daqp_amd {

// ---- the switches ------------------------------------------------------------------------------------------------------------------------
// how a switch's text becomes a value: kPresent -- set at all; kNonZero -- set to a non-zero integer; kInt / kLong -- atoi / atoll, taken
// ("on") only within [lo, hi], otherwise ignored as if it were not set (a use site may narrow the range further: WG_CAPL, WG_R0)
enum SwitchParse { kPresent, kNonZero, kInt, kLong };
// X(name behind DAQP_AMD_, parse, lo, hi, part of the pool key, read once per process)
// THE list of switches that shape a plan: read_tuning() reads exactly these, and the key under which a one-problem workspace is parked
// (Tuning::env_key) is their text -- a switch cannot be in one and not in the other.  (EXACT is not part of the key: a pooled workspace takes
// the caller's value when it is handed out, batch_create.  NO_SETUP_M, NO_BLK_SETUP and NO_BLK_BOUNDS are read by the setup path itself
// (daqp_amd.hip); they are listed for the key.  Not here, because they are read when a batch is solved, updated or freed: EAGER_UPDATE,
// NO_POOL, NO_EXIT_SYNC, RECHECK_DEVICE.)
#define DAQP_AMD_SWITCHES(X)                                                                                                        \
    X(LDS_LIMIT, kInt, INT_MIN, INT_MAX, 1, 0)           /* bytes of LDS beyond which k_ldp keeps its active rows in HBM (80 KB) */    \
    X(FORCE_SPILL, kPresent, 0, 0, 1, 0)                                                                                            \
    X(STREAM_M, kPresent, 0, 0, 1, 0)                    /* no register shape, no image: M streamed */                               \
    X(NO_WG, kPresent, 0, 0, 1, 0)                                                                                                  \
    X(WG_WAVES, kInt, 4, kWgMaxWaves, 1, 0)                                                                                         \
    X(WG_CAPL, kInt, 2, INT_MAX, 1, 0)                   /* (tests: force the hand-over) applies below the capL the LDS allows */    \
    X(WG_GRID, kLong, 1, LLONG_MAX, 1, 0)                /* tuning: problems in flight */                                            \
    X(NO_WG_TIER, kPresent, 0, 0, 1, 0)                                                                                             \
    X(WG_R0, kInt, 8, INT_MAX, 1, 0)                     /* (tests: more rows in the HBM tier) applies below the r0 half the LDS allows */ \
    X(WG_TIER_GRID, kLong, 1, LLONG_MAX, 1, 0)                                                                                      \
    X(WG_TIER_MIN_BATCH, kLong, 1, LLONG_MAX, 1, 0)      /* (tests: small batches through the tiered launch) */                      \
    X(SLOW_SETUP, kPresent, 0, 0, 1, 0)                                                                                             \
    X(NO_SCAN32, kPresent, 0, 0, 1, 0)                                                                                              \
    X(WG_INVERSE, kInt, 0, 0, 1, 0)                      /* "0": the workgroup kernel carries L, not L^-1 */                         \
    X(NO_TINY_SETUP, kPresent, 0, 0, 1, 0)                                                                                          \
    X(NO_RECHECK, kNonZero, 0, 0, 1, 0)                  /* no second pass over INFEASIBLE verdicts */                               \
    X(NO_SETUP_M, kNonZero, 0, 0, 1, 1)                                                                                             \
    X(NO_BLK_SETUP, kNonZero, 0, 0, 1, 1)                                                                                           \
    X(REG_ROWS, kInt, 1, 63, 1, 0)                       /* tests: force the hand-over */                                            \
    X(NO_REG_HANDOVER, kPresent, 0, 0, 1, 0)                                                                                        \
    X(NO_FACT_WG, kPresent, 0, 0, 1, 0)                                                                                             \
    X(NO_FACT_SMALL, kPresent, 0, 0, 1, 0)                                                                                          \
    X(NO_IMG32, kPresent, 0, 0, 1, 0)                                                                                               \
    X(IMG_ROWS, kInt, 2, 64, 1, 0)                                                                                                  \
    X(IMG_MIN_BATCH, kInt, INT_MIN, INT_MAX, 1, 0)                                                                                  \
    X(IMG_WAVES, kInt, 1, 8, 1, 0)                                                                                                  \
    X(IMG_CACHE, kInt, 1, INT_MAX, 1, 0)                                                                                            \
    X(IMG_WARM_ROWS, kInt, INT_MIN, INT_MAX, 1, 0)                                                                                  \
    X(IMG_WARM_WAVES, kInt, 1, 8, 1, 0)                                                                                             \
    X(NO_IMG_ONLY, kPresent, 0, 0, 1, 0)                                                                                            \
    X(IMG_ONLY_MIN_BATCH, kInt, INT_MIN, INT_MAX, 1, 0)                                                                             \
    X(NO_BLK_BOUNDS, kPresent, 0, 0, 1, 0)                                                                                          \
    X(EXACT, kNonZero, 0, 0, 0, 0)                       /* the reference's arithmetic (bit-exact LDP); default: fused multiply-adds, MFMA */ \
    X(NO_MAPPED_RESULTS, kNonZero, 0, 0, 0, 1)           /* one problem: results through a device slab and a copy, not mapped host memory */

enum Switch {
#define DAQP_AMD_SWITCH_ENUM(name, parse, lo, hi, key, once) SW_##name,
    DAQP_AMD_SWITCHES(DAQP_AMD_SWITCH_ENUM)
#undef DAQP_AMD_SWITCH_ENUM
    kSwitches
};
struct SwitchRule { const char *name; SwitchParse parse; long long lo, hi; bool key, once; };
inline const SwitchRule *switch_rules()
{
    static const SwitchRule rules[kSwitches] = {
#define DAQP_AMD_SWITCH_RULE(name, parse, lo, hi, key, once) {"DAQP_AMD_" #name, parse, lo, hi, key != 0, once != 0},
        DAQP_AMD_SWITCHES(DAQP_AMD_SWITCH_RULE)
#undef DAQP_AMD_SWITCH_RULE
    };
    return rules;
}
struct Tuning {
    struct Value { bool present = false, on = false; long long v = 0; } sw[kSwitches];
    std::string env_key;      // the text of every switch of the pool key, in the table's order
    bool present(Switch s) const { return sw[s].present; }
    bool on(Switch s) const { return sw[s].on; }
    long long val(Switch s, long long otherwise) const { return sw[s].on ? sw[s].v : otherwise; }
};
inline Tuning::Value parse_switch(const SwitchRule &r, const char *e)
{
    Tuning::Value v;
    if (!e) return v;
    v.present = true;
    if (r.parse == kPresent) { v.on = true; return v; }
    v.v = r.parse == kLong ? atoll(e) : (long long)atoi(e);
    v.on = r.parse == kNonZero ? v.v != 0 : (v.v >= r.lo && v.v <= r.hi);
    return v;
}
// the environment as it is NOW (every create reads it again), but for the switches that a process reads once
inline Tuning read_tuning()
{
    struct Once { Tuning::Value sw[kSwitches]; };      // (plain values: nothing of the library's is destroyed when the process exits)
    static const Once first = [] {
        Once o;
        for (int s = 0; s < kSwitches; ++s) o.sw[s] = parse_switch(switch_rules()[s], getenv(switch_rules()[s].name));
        return o;
    }();
    Tuning t;
    for (int s = 0; s < kSwitches; ++s) {
        const SwitchRule &r = switch_rules()[s];
        const char *e = getenv(r.name);
        t.sw[s] = r.once ? first.sw[s] : parse_switch(r, e);
        if (r.key) { t.env_key += e ? e : "-"; t.env_key += '|'; }
    }
    return t;
}

// ---- the plan ------------------------------------------------------------------------------------------------------------------------------
struct SolvePlan {
    int N = 0, n = 0, m = 0, ms = 0, ns_max = 0;
    int cap = 0, npair = 0, nblk = 0, nquad = 0, ldr = 0, ltri = 0, rtri = 0;
    int C = 1;                   // 64-row chunks of the one-wave kernel k_ldp
    bool spill = false;          // ... whose active rows live in HBM (rowc_g)
    int NB = 0, NP = 0;          // register-resident M variant (0: stream M from HBM)
    int reg_rows = 64;           // working-set rows a register kernel may hold (BatchDev::reg_rows)
    bool reg_handover = false;   // k_ldp_reg<2,32,*> may flag problems (more working-set rows than lanes: n = 64) for k_ldp right behind it
    size_t lds_fb = 0;           // ... and that launch's LDS
    bool img32 = false;          // default arithmetic: the solve launch is k_ldp_reg<NB, NP, true, 1> -- an fp32 image of M in the registers, two waves per
                                 // SIMD, at most img_rows working-set rows -- with k_ldp_reg<NB, NP, true, 0> right behind it for the problems it flags
    int img_kind = 0;            // its IMG template argument (2: the last row block split over two lanes per row; 1: full blocks)
    int img_rows = 0, img_cache = 0;   // rows the image kernel holds at all, and those of them in LDS (BatchDev::img_rows, img_cache)
    size_t lds_img = 0;          // ... and the image kernel's LDS
    // the carve-up of a WARM launch (daqp_update_ldp(UPDATE_v|UPDATE_d) fused into the solve: an MPC step starts from ~20 rows and moves a few): fewer
    // rows held at all, so that at the same eight workgroups per CU more of them sit in LDS (the launch argument carries rows | cache, see k_ldp_reg)
    int img_rows_warm = 0, img_cache_warm = 0;
    size_t lds_img_warm = 0;
    bool img_only = false;       // no register shape holds M, but its fp32 image fits (k_ldp_reg<NB,NP,true,1> of kImgOnlyShapes, one wave per SIMD): default-mode solves run it in front of k_ldp
    int io_nb = 0, io_np = 0;
    int img_min_warm = 16384;    // warm launches take the image kernel from this batch size on
    int ldrc = 0;                // row stride of the register kernels' active-row cache (BatchDev::ldrc)
    // workgroup-per-problem solve kernel (wg_kernel.hip.h): shapes without a register variant and more than 64 working-set rows
    bool use_wg = false;
    int wg_W = 0, wg_C = 0, wg_inverse = 0, wg_capL = 0, wg_capT = 0;
    size_t lds_wg = 0;
    int wg_grid = 0;                                              // (plan_device)
    int wg_r0 = 0, wg_tier_grid = 0; size_t lds_wg_tier = 0;      // tiered launch of the workgroup kernel in front of a cold solve (0: none; plan_device)
    bool tiny_setup = false;     // n <= 12, m <= 48: the 16-problems-per-wave setup kernel (tiny_setup.hip.h)
    bool fast_setup = false, setup_spill = false;
    bool fact_gs = false;        // 64 < n, factors that WOULD fit the LDS of k_setup: the default arithmetic's full setup still takes k_fact_wg + the scratch variant
    size_t lds_setup = 0, lds_ldp = 0, lds_update = 0;
    int exact_setup = 0;         // the arithmetic a new batch starts in (BatchDev::exact_setup; daqp_batch_set_exact changes the batch, not the plan)
    // which buffers exist besides the ones every batch has (group > 1: groups of `group` consecutive problems share one set of factors, and such a
    // batch is never set up from H / A: the scratch of the QP setup kernels stays away)
    int factor_sets = 0;         // sets of Mblk / M32 / R^-1 / scaling
    bool has_setup_g = false, has_m32 = false, has_setup_sq = false, has_fact_buf = false;
    bool mapped_results = true;  // one problem: the result slab is mapped host memory
};

#ifndef DAQP_AMD_PLAN_TYPES_ONLY
constexpr int kPlanWhy = 256;    // bytes of a refusal's text
inline bool plan_dims_ok(int N, int n, int m, int ms, int ns_max, char *why)
{
    if (N <= 0 || n <= 0 || m < 0 || ms < 0 || ms > m || ms > n || ns_max < 0) {
        snprintf(why, kPlanWhy, "bad dimensions N=%d n=%d m=%d ms=%d ns=%d", N, n, m, ms, ns_max);
        return false;
    }
    const int cap = n + ns_max + 1;
    if (cap > 512 || n > 511) { snprintf(why, kPlanWhy, "n + ns + 1 = %d exceeds the 512-row working-set limit of this build", cap); return false; }
    return true;
}

// register-resident variants: (row blocks, k-pairs) held per lane; needs cap <= 64 and L/rows in LDS
struct RegShape { int nb, np; };
#ifdef DAQP_AMD_FEW_VARIANTS   // development builds: fewer instantiations, faster compile
const RegShape kRegShapes[] = {{1, 6}, {1, 8}, {3, 25}};
#else
const RegShape kRegShapes[] = {{1, 6}, {1, 8}, {1, 13}, {1, 16}, {2, 16}, {3, 8}, {4, 8}, {1, 25}, {3, 25}, {2, 32}};   // ((3,8), (4,8): few variables, many rows -- n <= 16, m <= 192; (1,25): n <= 50 with m <= 64 -- both at two waves per SIMD)
#endif
// the shapes served by an fp32 image ALONE (no full-register kernel exists: M itself would not fit 512 registers), first fit:
// (4,32) n <= 63, m <= 256 | (8,16) n <= 32, m <= 512 | (6,25) n <= 50, m <= 384 | (5,32) n <= 63, m <= 320 -- 256 ... 320 image registers, one wave per SIMD
const RegShape kImgOnlyShapes[] = {{4, 32}, {8, 16}, {6, 25}, {5, 32}};

// stride == 2 (mod 4): rows 16-byte aligned and 16 consecutive rows hit 16 distinct 4-bank groups
inline int reg_cache_stride(int n, int np)
{
    int l = n > 2 * np ? n : 2 * np;
    while ((l & 3) != 2) ++l;
    return l;
}
// rows of the image kernels' active-row cache in LDS: as many of `rows` as leave `waves` workgroups per CU (the rest of a working set lives in
// rowc_g, L2-resident); a workgroup's share of the CU's 160 KB is granted in 512-byte steps
inline int img_cache_rows(int nb, int kind, int n, int m, int rows, int ldrc, int waves)
{
    const int budget = (160 * 1024 / waves) / 512 * 512;
    int cache = rows;
    while (cache > 2 && reg_img_lds_bytes(nb, kind, n, m, rows, cache, ldrc) > budget) --cache;
    return cache;
}

// Stage 1: everything a shape and the switches decide.  false: the shape is refused, `why` (kPlanWhy bytes) says so.
inline bool plan_shape(int N, int n, int m, int ms, int ns_max, int group, const Tuning &T, SolvePlan *out, char *why)
{
    if (!plan_dims_ok(N, n, m, ms, ns_max, why)) return false;
    SolvePlan p;
    const int cap = n + ns_max + 1;
    p.N = N; p.n = n; p.m = m; p.ms = ms; p.ns_max = ns_max; p.cap = cap;
    p.npair = (n + 1) / 2; p.nblk = (m + 63) / 64; p.ldr = n | 1; p.nquad = (p.npair + 1) / 2;
    p.ltri = round_up(cap * (cap + 1) / 2, 2); p.rtri = n * (n + 1) / 2;   // even stride: 16-byte aligned rows for the direct HBM->LDS copy
    p.C = cap <= 64 ? 1 : (cap <= 128 ? 2 : (cap <= 256 ? 4 : 8));
#ifdef DAQP_AMD_FEW_VARIANTS
    if (p.C < 4) p.C = 4;
#endif
    const int lds_limit = (int)T.val(SW_LDS_LIMIT, 80 * 1024);
    p.spill = ldp_lds(n, m, cap, false).total_bytes > lds_limit;
    if (T.on(SW_FORCE_SPILL) || cap > 256) p.spill = true;
    if (!p.spill && cap <= 65 && !T.on(SW_STREAM_M))
        for (const RegShape &rs : kRegShapes)
            if (p.nblk <= rs.nb && p.npair <= rs.np) { p.NB = rs.nb; p.NP = rs.np; break; }
    // one lane per working-set row: 64 rows.  n = 64 without soft rows may hold 65 (only while a 65th constraint is being exchanged at a full
    // vertex): the (2,32) shape takes it and hands the few problems that get there to k_ldp (launch_ldp); every other shape needs cap <= 64
    p.reg_rows = (int)T.val(SW_REG_ROWS, 64);
    if (p.NB > 0 && p.reg_rows < cap) {
        if (p.NB == 2 && p.NP == 32 && !T.on(SW_NO_REG_HANDOVER)) p.reg_handover = true;
        else if (cap > 64) { p.NB = 0; p.NP = 0; }
    }
    if (p.reg_handover) p.lds_fb = (size_t)ldp_lds(n, m, cap, p.spill).total_bytes;
    // The shapes whose M fills the register file (one wave per SIMD) run, in the default arithmetic and on batches that fill the device twice
    // over, as an fp32 IMAGE of M at two waves per SIMD (reg_kernel.hip.h, IMG = 1).  Its LDS holds img_rows working-set rows (C2: the peak is
    // 27 rows on average, above 40 on 1.3 % of the problems -- those are handed to the full-register kernel behind it)
    p.img_kind = (p.NB == 3 && p.NP == 25) ? (m <= 160 ? 2 : 1) : ((p.NB == 2 && p.NP == 32) ? 1 : 0);
    if (p.img_kind && cap <= 64 && !p.reg_handover && !T.on(SW_NO_IMG32)) {
        // (tools/img_threshold.py: below ~10 000 problems -- warm launches: ~16 000, see launch_ldp -- the device is not full twice over and a problem's latency decides: one wave per SIMD is faster per problem)
        const int min_batch = (int)T.val(SW_IMG_MIN_BATCH, 10240), rows = (int)T.val(SW_IMG_ROWS, 42);
        if (T.present(SW_IMG_MIN_BATCH)) p.img_min_warm = min_batch;      // (the tests' override applies to every launch)
        if (N >= min_batch) { p.img32 = true; p.img_rows = rows < cap ? rows : cap; }
    }
    if (p.NB > 0) p.ldrc = reg_cache_stride(n, p.NP);
    p.lds_ldp = p.NB > 0 ? (size_t)reg_lds_bytes(p.NB, n, m, cap, p.ldrc) : (size_t)ldp_lds(n, m, cap, p.spill, p.ldrc).total_bytes;
    // No register shape for (n, m), but the fp32 image of M fits one (kImgOnlyShapes: n <= 63 with m <= 256 ... 512, one wave per SIMD): the default
    // arithmetic's solves run on it (launch_ldp); everything else about the batch stays the generic one-wave path's.  Every working-set row the
    // shape can have is held (img_rows = cap), as many of them in LDS as leave four workgroups per CU, the rest in the scratch tier.
    // (n <= 16: M streamed is as fast -- n = 8, m = 256: 0.86 against 1.02 ms per 20 000 -- a scan is 16 column pairs of L2 hits)
    int io_nb = 0, io_np = 0;
    for (const RegShape &rs : kImgOnlyShapes)
        if (p.nblk <= rs.nb && p.npair <= rs.np) { io_nb = rs.nb; io_np = rs.np; break; }
    // (cap = 65 is n = 64 without soft rows: a 65th row exists only while a constraint is exchanged at a full vertex -- the image kernel holds 64
    //  and flags such a problem for k_ldp behind it, as the (2,32) registers do for m <= 128)
    // (n = 64 with m <= 128 keeps its (2,32) registers for the exact mode, fused updates and one-problem calls; the default arithmetic's plain
    //  solves of a batch take the image-only kernel there as well: 6.5 -> 4.0 ms per 20 000 at m = 128 -- the fp32 scan is half the issue slots)
    const bool n64 = p.NB == 2 && p.NP == 32 && p.reg_handover && N > 1;
    if ((p.NB == 0 || n64) && !p.spill && n > 16 && cap <= 65 && n <= 64 && io_nb > 0 && !T.on(SW_STREAM_M) && !T.on(SW_NO_IMG32) && !T.on(SW_NO_IMG_ONLY)) {
        if (N >= (int)T.val(SW_IMG_ONLY_MIN_BATCH, 1)) {
            p.img_only = true; p.io_nb = io_nb; p.io_np = io_np;
            p.ldrc = reg_cache_stride(n, io_np);      // (the row-cache stride of the register kernels; k_ldp has its own)
            p.img_rows = cap < 64 ? cap : 64;
            p.img_cache = img_cache_rows(io_nb, 1, n, m, p.img_rows, p.ldrc, 4);
            p.lds_img = (size_t)reg_img_lds_bytes(io_nb, 1, n, m, p.img_rows, p.img_cache, p.ldrc);
        }
    }
    if (p.img32) {
        const int waves = (int)T.val(SW_IMG_WAVES, 8);
        int cache = img_cache_rows(p.NB, p.img_kind, n, m, p.img_rows, p.ldrc, waves);
        if (T.on(SW_IMG_CACHE)) { const int v = (int)T.val(SW_IMG_CACHE, 0); cache = v < p.img_rows ? v : p.img_rows; }
        p.img_cache = cache;
        p.lds_img = (size_t)reg_img_lds_bytes(p.NB, p.img_kind, n, m, p.img_rows, cache, p.ldrc);
        if (!T.present(SW_IMG_ROWS) && !T.present(SW_IMG_CACHE)) {      // (the tests' overrides apply to every launch)
            const int wrows = (int)T.val(SW_IMG_WARM_ROWS, 40);
            if (wrows >= 2 && wrows < p.img_rows) {
                p.img_rows_warm = wrows;
                p.img_cache_warm = img_cache_rows(p.NB, p.img_kind, n, m, wrows, p.ldrc, (int)T.val(SW_IMG_WARM_WAVES, waves));
                p.lds_img_warm = (size_t)reg_img_lds_bytes(p.NB, p.img_kind, n, m, wrows, p.img_cache_warm, p.ldrc);
            }
        }
    }
    if (p.NB == 0 && !p.img_only && cap > 64 && cap <= 256 && !T.on(SW_NO_WG)) {     // (beyond 256 rows: the one-wave kernel with eight chunks, everything large in HBM scratch)
        int W = p.nblk < 4 ? 4 : (p.nblk > kWgMaxWaves ? kWgMaxWaves : p.nblk);
        const int lds_max = 160 * 1024 - 512;          // (the kernel's static LDS -- 320 bytes by the code generator's report -- comes on top of the
                                                       //  dynamic allocation: with 256 bytes of reserve a shape whose packed factor ended within 64 bytes
                                                       //  of the limit, (n, m) = (187, 371), could not be launched at all)
        const int Cw = cap <= 128 ? 2 : 4;
        // Two workgroups per CU beat one with more waves wherever the whole factor fits half the LDS: one problem's serial master phases then run
        // under the other's bandwidth phases (n = 100, m = 300: solve launch 29.8 -> 17.9 ms per 4 096; n = 110, m = 330: 17.1 -> 10.8 ms,
        // profiles/r06t_wg_two_per_cu.txt).  The register file holds eight waves per CU, so two workgroups means four waves each.
        if (W > 4 && wg_lds_bytes(Cw, m, cap) <= lds_max / 2 - 256) W = 4;
        W = (int)T.val(SW_WG_WAVES, W);
        int capL = cap;
        while (capL > 16 && wg_lds_bytes(Cw, m, capL) > lds_max) --capL;
        if (T.on(SW_WG_CAPL) && T.val(SW_WG_CAPL, 0) < capL) capL = (int)T.val(SW_WG_CAPL, 0);   // (tests: force the hand-over)
        if (wg_lds_bytes(Cw, m, capL) <= lds_max && capL >= (cap < 48 ? cap : 48)) {
            p.use_wg = true; p.wg_W = W; p.wg_C = Cw;
            p.wg_inverse = T.on(SW_WG_INVERSE) ? 0 : 1;   // default mode: L^-1 instead of L (wg_ldp.hip.h)
            p.wg_capL = capL; p.wg_capT = round_up(cap, 8);
            p.lds_wg = (size_t)wg_lds_bytes(Cw, m, capL);
        }
    }
    p.fast_setup = (n <= 64) && !T.on(SW_SLOW_SETUP);
    p.tiny_setup = p.fast_setup && n <= TNC && m <= TMR && !T.on(SW_NO_TINY_SETUP);
    p.exact_setup = T.on(SW_EXACT) ? 1 : 0;   // DAQP_AMD_EXACT=1: keep the reference's summation order in M = A R^-1 (bit-exact LDP); default: MFMA
    p.setup_spill = !p.fast_setup && (setup_lds(n, m).total_bytes > 150 * 1024 || T.on(SW_FORCE_SPILL) || n > 256);
    p.lds_setup = p.fast_setup ? (size_t)fast_lds(n, m, 1, m - ms).total_bytes : (size_t)setup_lds(n, m, p.setup_spill).total_bytes;
    // 64 < n <= ~134: both factors fit the LDS of k_setup, where ONE wave factors and inverts in the reference's order -- 13.5 ms per 4 096 problems at
    // n = 100 against 5.2 ms at n = 150, where k_fact_wg (a workgroup per problem, matrix cores) does it.  The default arithmetic's full setup takes
    // k_fact_wg + the scratch variant of k_setup for these shapes too (profiles/r06v_shape_map.txt -> r06w); exact mode, partial updates and the
    // regularising passes keep the LDS variant.
    p.fact_gs = !p.fast_setup && !p.setup_spill && n > 64 && n <= kFactMaxN && !T.on(SW_NO_FACT_WG) && !T.on(SW_NO_FACT_SMALL);
    p.lds_update = (size_t)round_up(n, 2) * 16;
    if (p.lds_ldp > 160 * 1024 || p.lds_setup > 160 * 1024) {
        snprintf(why, kPlanWhy, "problem too large for the LDS-staged setup (needs %zu / %zu bytes)", p.lds_setup, p.lds_ldp);
        return false;
    }
    p.factor_sets = group > 1 ? (N + group - 1) / group : N;
    p.has_setup_g = (p.setup_spill || p.fact_gs) && group <= 1;
    p.has_m32 = p.use_wg && !p.fast_setup && !T.on(SW_NO_SCAN32);     // fp32 image of M for the workgroup kernel's screening scan (generic setup kernel only: it is the one that writes it)
    p.has_setup_sq = !p.fast_setup && group <= 1;
    p.has_fact_buf = p.has_setup_sq && (p.setup_spill || p.fact_gs) && n <= kFactMaxN && !T.on(SW_NO_FACT_WG);
    p.mapped_results = !T.on(SW_NO_MAPPED_RESULTS);
    *out = p;
    return true;
}

// Stage 2, for the shapes of the workgroup kernel (stage 1 chose it: wg_W > 0): its grid, and the tiered launch.  The device's facts enter as
// numbers: its CU count, the workgroups of k_ldp_wg<wg_C> (64 wg_W threads, lds_wg bytes) that fit one CU, whether k_ldp_wg<wg_C, false, true>
// accepts the tier's LDS, and how many of its workgroups (256 threads) fit one CU.  The last two can only be asked once the tier's rows are
// known: plan_wg_grid says whether and for what (TierQuery), plan_wg_tier takes the answer; plan_device is the two in a row.
struct TierQuery { int r0 = 0; size_t lds = 0; };
inline bool plan_wg_grid(SolvePlan *p, const Tuning &T, int cus, int per_cu, TierQuery *q)
{
    if (per_cu < 1) per_cu = 1;
    const long long g = T.val(SW_WG_GRID, (long long)cus * per_cu);
    p->wg_grid = (int)(g < p->N ? g : p->N);
    // Tiered launch (wg_kernel.hip.h, TIER): where the whole factor allows only one workgroup per CU, cold solves run two four-wave workgroups
    // per CU with the rows of the inverse factor beyond what half the LDS holds in HBM.  Worth it only while enough problems are in flight.
    const long long tier_min = T.val(SW_WG_TIER_MIN_BATCH, 2LL * cus);
    if (!(p->use_wg && per_cu == 1 && p->wg_inverse && !T.on(SW_NO_WG_TIER) && p->N >= tier_min)) return false;
    const int half = (160 * 1024 - 512) / 2 - 256;
    int r0 = p->cap;
    while (r0 > 16 && wg_lds_bytes(p->wg_C, p->m, r0) > half) --r0;
    if (T.on(SW_WG_R0) && T.val(SW_WG_R0, 0) < r0) r0 = (int)T.val(SW_WG_R0, 0);    // (tests: more rows in the HBM tier)
    q->r0 = r0; q->lds = (size_t)wg_lds_bytes(p->wg_C, p->m, r0);
    return r0 >= 32 && r0 < p->cap;
}
inline void plan_wg_tier(SolvePlan *p, const Tuning &T, int cus, const TierQuery &q, bool tier_attr_ok, int per_cu_tier)
{
    if (!tier_attr_ok || per_cu_tier < 2) return;
    p->wg_r0 = q.r0; p->lds_wg_tier = q.lds;
    const long long g2 = T.val(SW_WG_TIER_GRID, (long long)cus * per_cu_tier);
    p->wg_tier_grid = (int)(g2 < p->N ? g2 : p->N);
}
inline void plan_device(SolvePlan *p, const Tuning &T, int cus, int per_cu, bool tier_attr_ok, int per_cu_tier)
{
    TierQuery q;
    if (p->wg_W > 0 && plan_wg_grid(p, T, cus, per_cu, &q)) plan_wg_tier(p, T, cus, q, tier_attr_ok, per_cu_tier);
}

#endif   // DAQP_AMD_PLAN_TYPES_ONLY

// what the descriptor carries of the plan
inline void plan_fill(const SolvePlan &p, BatchDev *d)
{
    d->N = p.N; d->n = p.n; d->m = p.m; d->ms = p.ms; d->cap = p.cap; d->mA = p.m - p.ms;
    d->npair = p.npair; d->nblk = p.nblk; d->ldr = p.ldr; d->nquad = p.nquad; d->ltri = p.ltri; d->rtri = p.rtri;
    d->reg_rows = p.reg_rows; d->img_rows = p.img_rows; d->img_cache = p.img_cache; d->ldrc = p.ldrc;
    d->wg_inverse = p.wg_inverse; d->wg_capL = p.wg_capL; d->wg_capT = p.wg_capT; d->wg_r0 = p.wg_r0;
    d->exact_setup = p.exact_setup;
}

// ---- the launch sequence of a solve ------------------------------------------------------------------------------------------------------
enum SolvePath {
    kPathWg,             // k_ldp_wg, k_ldp behind it for what outgrows the LDS-resident factor
    kPathWgTier,         // ... with the tiered launch in front (a first solve in the default arithmetic)
    kPathReg,            // k_ldp_reg
    kPathRegImg,         // the fp32-image kernel, k_ldp_reg behind it for the working sets it does not hold
    kPathN64ImgOnly,     // n = 64 in the default arithmetic: the image-only kernel, k_ldp behind it for a 65th row
    kPathRegHandover,    // k_ldp_reg<2,32>, k_ldp behind it for the problems it flags
    kPathWave,           // k_ldp
    kPathWaveImgOnly,    // the image-only kernel, k_ldp behind it
};
// mode: the launch's (0: solve; 1: activate from sense; 2 | mask << 4: fused update + solve; | 4: flagged problems only).  exact_kernels: the
// reference's arithmetic (the batch's mode, the proximal outer loop, a sticky working set).  fresh: nothing solved or updated since the setup.
// img_allowed: what only the launch knows about the image kernel -- most of the last launch was handed over, a warm batch below img_min_warm
inline SolvePath pick_path(const SolvePlan &p, int mode, bool exact_kernels, bool fresh, bool img_allowed)
{
    if (p.use_wg) return (p.wg_tier_grid > 0 && fresh && mode == 0 && !exact_kernels) ? kPathWgTier : kPathWg;
    if (p.NB > 0) {
        if (p.img32 && !exact_kernels && img_allowed) return kPathRegImg;
        if (p.reg_handover && p.img_only && mode == 0 && !exact_kernels) return kPathN64ImgOnly;
        return p.reg_handover ? kPathRegHandover : kPathReg;
    }
    return (p.img_only && mode == 0 && !exact_kernels) ? kPathWaveImgOnly : kPathWave;
}

// ---- the read-out (daqp_amd_describe_plan, daqp_batch_describe): one line, fixed key order ---------------------------------------------------
inline int describe_plan(const SolvePlan &p, char *buf, int len)
{
    // paths=: pick_path's answer as a digit (SolvePath) for mode 0, 1, 2 x exact_kernels 0, 1 x fresh 0, 1 x img_allowed 0, 1, in that nesting
    char paths[25];
    for (int i = 0; i < 24; ++i) paths[i] = (char)('0' + pick_path(p, i >> 3, (i >> 2 & 1) != 0, (i >> 1 & 1) != 0, (i & 1) != 0));
    paths[24] = 0;
    return snprintf(buf, (size_t)len,
        "N=%d n=%d m=%d ms=%d ns_max=%d cap=%d npair=%d nblk=%d nquad=%d ldr=%d ltri=%d rtri=%d C=%d spill=%d NB=%d NP=%d reg_rows=%d reg_handover=%d lds_fb=%zu "
        "img32=%d img_kind=%d img_rows=%d img_cache=%d lds_img=%zu img_rows_warm=%d img_cache_warm=%d lds_img_warm=%zu img_only=%d io_nb=%d io_np=%d img_min_warm=%d ldrc=%d "
        "use_wg=%d wg_W=%d wg_C=%d wg_inverse=%d wg_capL=%d wg_capT=%d lds_wg=%zu wg_grid=%d wg_r0=%d wg_tier_grid=%d lds_wg_tier=%zu "
        "tiny_setup=%d fast_setup=%d setup_spill=%d fact_gs=%d lds_setup=%zu lds_ldp=%zu lds_update=%zu exact_setup=%d "
        "factor_sets=%d has_setup_g=%d has_m32=%d has_setup_sq=%d has_fact_buf=%d mapped_results=%d paths=%s",
        p.N, p.n, p.m, p.ms, p.ns_max, p.cap, p.npair, p.nblk, p.nquad, p.ldr, p.ltri, p.rtri, p.C, (int)p.spill, p.NB, p.NP, p.reg_rows, (int)p.reg_handover, p.lds_fb,
        (int)p.img32, p.img_kind, p.img_rows, p.img_cache, p.lds_img, p.img_rows_warm, p.img_cache_warm, p.lds_img_warm, (int)p.img_only, p.io_nb, p.io_np, p.img_min_warm, p.ldrc,
        (int)p.use_wg, p.wg_W, p.wg_C, p.wg_inverse, p.wg_capL, p.wg_capT, p.lds_wg, p.wg_grid, p.wg_r0, p.wg_tier_grid, p.lds_wg_tier,
        (int)p.tiny_setup, (int)p.fast_setup, (int)p.setup_spill, (int)p.fact_gs, p.lds_setup, p.lds_ldp, p.lds_update, p.exact_setup,
        p.factor_sets, (int)p.has_setup_g, (int)p.has_m32, (int)p.has_setup_sq, (int)p.has_fact_buf, (int)p.mapped_results, paths);
}

} // namespace daqp_amd

// ---- the kernels behind a plan: for the unit that launches them (daqp_amd.hip, which declares the instantiations of the other units first) ----
#ifdef DAQP_AMD_PLAN_KERNELS
namespace daqp_amd {
typedef void (*ldp_kernel_t)(BatchDev, int);
typedef void (*ldp_reg_kernel_t)(const BatchDev *, int);
inline ldp_reg_kernel_t pick_img_only(const SolvePlan &p)
{
    if (p.io_nb == 4 && p.io_np == 32) return k_ldp_reg<4, 32, true, 1>;
    if (p.io_nb == 8 && p.io_np == 16) return k_ldp_reg<8, 16, true, 1>;
    if (p.io_nb == 6 && p.io_np == 25) return k_ldp_reg<6, 25, true, 1>;
    if (p.io_nb == 5 && p.io_np == 32) return k_ldp_reg<5, 32, true, 1>;
    return nullptr;
}
// exact: the reference's arithmetic (two roundings per multiply-add); otherwise fused multiply-adds (default mode)
inline ldp_reg_kernel_t pick_ldp_reg_img(const SolvePlan &p)
{
    if (p.NB == 3 && p.NP == 25) return p.img_kind == 2 ? k_ldp_reg<3, 25, true, 2>      // (IMG = 2: the third row block holds at most 32 rows)
                                                         : k_ldp_reg<3, 25, true, 1>;     // (161 <= m <= 192: three full blocks, 150 image registers, 23 of the rest in scratch)
    if (p.NB == 2 && p.NP == 32) return k_ldp_reg<2, 32, true, 1>;    // (51 <= n <= 63, m <= 128: two full row blocks, 128 image registers)
    return nullptr;
}
inline ldp_reg_kernel_t pick_ldp_reg(const SolvePlan &p, bool exact)
{
#define DAQP_REG_PICK(nb, np) if (p.NB == nb && p.NP == np) return exact ? k_ldp_reg<nb, np, false> : k_ldp_reg<nb, np, true>;
    DAQP_REG_PICK(1, 6)
    DAQP_REG_PICK(1, 8)
    DAQP_REG_PICK(3, 25)
#ifndef DAQP_AMD_FEW_VARIANTS
    DAQP_REG_PICK(1, 13)
    DAQP_REG_PICK(1, 16)
    DAQP_REG_PICK(2, 16)
    DAQP_REG_PICK(3, 8)
    DAQP_REG_PICK(4, 8)
    DAQP_REG_PICK(1, 25)
    DAQP_REG_PICK(2, 32)
#endif
#undef DAQP_REG_PICK
    return nullptr;
}
inline ldp_kernel_t pick_ldp(const SolvePlan &p)
{
    const int C = p.C;
    const bool spill = p.spill;
#ifdef DAQP_AMD_FEW_VARIANTS
    if (!spill) return k_ldp<4, false, 0, 0>;
    return C == 8 ? k_ldp<8, true, 0, 0> : k_ldp<4, true, 0, 0>;
#else
    if (!spill) {
        if (C == 1) return k_ldp<1, false, 0, 0>;
        if (C == 2) return k_ldp<2, false, 0, 0>;
        return k_ldp<4, false, 0, 0>;
    }
    if (C == 1) return k_ldp<1, true, 0, 0>;
    if (C == 2) return k_ldp<2, true, 0, 0>;
    if (C == 8) return k_ldp<8, true, 0, 0>;
    return k_ldp<4, true, 0, 0>;
#endif
}
} // namespace daqp_amd
#endif
