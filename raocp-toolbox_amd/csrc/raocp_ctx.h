// raocp_ctx.h -- the context behind the C-ABI (include/raocp_hip.h): struct raocp_ctx with its
// allocation / upload helpers, the error helpers (fail, HIPCHK) and the environment-switch
// readers. Self-contained (it names only types of raocp_common.h and of the launch headers), so
// any host unit of the library may include it: raocp_capi.hip and raocp_batch.hip do, through
// raocp_host.h. The helpers are inline and the error string is one inline variable: whichever
// unit fails, raocp_last_error() returns its message.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "raocp_common.h"
#include "raocp_dynr.h"
#include "raocp_cpb.h"
#include "raocp_eval.h"
#include "raocp_path.h"
#include "../../include/raocp_hip.h"

namespace raocp {

inline thread_local std::string g_err;

inline int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIPCHK(expr)                                                                             \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess)                                                                    \
            return fail(RAOCP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));       \
    } while (0)

inline int cdiv(int a, int b) { return b <= 0 ? 0 : (a + b - 1) / b; }

// CP iterations per captured graph: a multiple of 6 (buffer rotation period, see rotated())
constexpr int kGraphBatch = 24;

}  // namespace raocp

using raocp::Ctl;
using raocp::CpPath;
using raocp::DynPath;
using raocp::Dev;
using raocp::cdiv;
using raocp::fail;
using raocp::kGraphBatch;

struct raocp_ctx {
    int device = 0;
    bool f32 = false;            // RAOCP_F32: iterate, tables and products in fp32
    bool dyn32 = false;          // the per-stage T-templated dynamics (raocp_dyn2.hip) is planned
    bool ell3 = false;           // L by streaming wave tasks (raocp_ell3.hip)
    int ell3_grid = 0;
    int box_mode = 0;            // k_ell3 / k_ellt3: bits 0-1 nonleaf, 2-3 leaf boxes (1 all, 2 none, 0 mixed)
    int unif_C = 0;              // uniform branching factor <= 4 with uniform tables (0 = not)
    int unif_branch = 0;         // uniform branching factor <= 4 (children 1 + C i ..), any tables (dyn3)
    int ellt3_C = 0;             // L^T by streaming wave tasks: uniform branching factor (0 = off)
    int ellt3_grid = 0;
    bool cp3 = false;            // the CP iteration after the dynamics as one streaming kernel (raocp_cp3.hip)
    bool cp4 = false;            // ... with every operand of a tile loaded at its start (raocp_cp4.hip; RAOCP_CP4=0: off)
    int cp4_wpb = 2;             // k_cp4's waves per workgroup, one task per workgroup: 2 = helper mode (wave 1
                                 // takes a leaf-parent tile's leaf children), 1 = one wave (RAOCP_CP4_HELPER=0);
                                 // one task per workgroup spreads the load bursts over all CUs (round 4: one
                                 // task per wave at four waves per workgroup 18.5 vs 16.7 us at one)
    bool cp5 = false;            // ... as a leaf launch and a family launch (raocp_cp5.hip: configs 3, 4, 5;
                                 // RAOCP_CP5=0: off)
    bool cp6 = false;            // ... as one family tile per workgroup of 2 C waves (raocp_cp5.hip k_cp6: config
                                 // 2; RAOCP_CP6=0: k_cp4)
    int cp6_grid = 0;
    raocp::Cp3Tasks cp5_tk{};    // k_cp5_fam's / k_cp6's task list (every parent, leaf parents first)
    int cp5_gl = 0, cp5_gf = 0;  // grids of the two launches
    raocp::Cp3Tasks cp5_et{};    // k_cp5_leaf's eta2 tasks (nonleaf ranges, 64 nodes per task)
    raocp::Cp3Tasks cp5_tkb{};   // a shard's second k_cp5 launch: the cut's parents, after X1
    int cp5_gfb = 0;             // ... its grid
    bool cp5_lpf = false;        // k_cp5_leaf's form (RAOCP_CP5_LPF, raocp_cp5.h)
    int cp3_grid = 0;            // workgroups of the (first) k_cp3 launch
    int cp3_mL = 0;              // first parent whose children are leaves (stage N - 1)
    int cp3_split = 0;           // leaves as tasks of their own (small trees: more waves, shorter chains)
    raocp::Cp3Tasks cp3_ta{};    // the launch's task list (a shard: its own families + the top)
    raocp::Cp3Tasks cp3_tb{};    // a shard's second launch: the cut's parents, after X1
    int cp3_gridb = 0;
    double* cp3img = nullptr;    // k_cp3's weight fragments in LDS order (k_cp3_image)
    // per-stage MFMA dynamics (raocp_dyn2.hip): tables, node lists, tile lists per stage
    bool dyn2 = false;           // fp32 contexts always; fp64 opt-in RAOCP_DYN2=1
    const double *W2 = nullptr, *RG2 = nullptr, *KM2 = nullptr, *F2 = nullptr;
    const int* d2_idx = nullptr;
    const raocp::DynTile* d2_tiles = nullptr;
    std::vector<int> d2_off;     // per stage t: [prod, node, fwdU, fwdX] tile offsets, 5 entries
    double *Q2 = nullptr, *PA2 = nullptr, *Dd2 = nullptr;
    // per-stage streaming dynamics (raocp_dyn3.hip): uniform branching, per-slot kinds and one
    // class per stage; fp32 contexts by default, fp64 opt-in RAOCP_DYN3=1
    bool dyn3 = false;
    std::vector<raocp::Dy3Stage> d3st;
    double *d3img_b = nullptr, *d3img_f = nullptr;  // per-stage table images (k_dy3_image)
    std::vector<raocp::Dy3Stage> d3own;  // a shard's stages (owned parent ranges below its cut)
    int d3ts = 0;  // the top stages k_dy3_top_back / k_dy3_top_fwd run in one workgroup (0: none)
    size_t d3nb = 0, d3nf = 0;  // doubles per stage image (backward, forward)
    int wsz = 8;                 // bytes per scalar of the iterate
    hipStream_t stream = nullptr;
    Dev dev{};
    int n = 0, m = 0, nx = 0, nu = 0, cmax = 0, N = 0;
    std::vector<int> stage_ptr;  // start id of each stage, size N+2
    int64_t P = 0, D = 0;
    // iterate and work buffers
    double* Z[3] = {nullptr, nullptr, nullptr};
    double* E[2] = {nullptr, nullptr};
    double* XI2 = nullptr;
    double* q = nullptr;         // q rows of the cut stage, padded (n x KP)
    double* d = nullptr;         // d rows (m x nu)
    // per-stage dynamics path: padded global rows
    double* gXQ = nullptr;       // n x KP  (x, then q)
    double* gU = nullptr;        // m x NUP
    double* gXD = nullptr;       // m x KF  ([x | d | 0])
    double* gP = nullptr;        // n x PS  (child products)
    int KP = 0, KF = 0, NUP = 0, PS = 0;
    int maxch_top = 0;
    std::vector<int> cls_ptr;    // first class of each stage (size N+1)
    std::vector<int> pair_ptr;   // first (kind, class) pair of each class (size n_k+1)
    int nkind = 0;
    bool f_lds_top = false;      // F table staged in LDS by k_dyn_top
    bool fold_top = false;       // k_dyn_top's backward levels in one phase (WT tables)
    struct TierPlan {            // a tier [s0, s1) below the top: one workgroup per subtree
        int s0, s1, nsub, maxch;
        size_t lds_b, lds_f;
        int fm;                  // F in the forward kernel: 0 global, 1 LDS, 2 LDS per level
        bool fold;               // one-phase backward levels (WT tables)
        const raocp::Rec* lv;    // level ranges of its subtrees
        raocp::TierArg ta;       // the same, as a kernel argument, when the tier is regular
    };
    std::vector<TierPlan> tiers;
    raocp::FuseArg fuse{};       // the split sweep's plan (counters / flags in fuse_sync)
    bool dyn_split = false;      // the tiered sweep in TWO launches (k_dyn_up / k_dyn_down)
    size_t lds_up = 0, lds_down = 0;
    unsigned* fuse_sync = nullptr;  // [epoch | error word | per tier: counters, flags]
    size_t fuse_words = 0;
    // the regular-tree sweep (raocp_dynr.hip): two launches, one workgroup per subtree of
    // every tier; the default for fp64 regular trees of the compiled sizes (RAOCP_DR=0: off)
    bool reg_ok = false;            // uniform branching, one class per stage, one pair per slot
    int reg_C = 0;
    std::vector<raocp::Dy3Stage> reg_st;
    bool dr = false;
    raocp::DrPlan drp{};
    int dr_block = 512;
    size_t dr_lds = 0;
    // k_drc (raocp_dynr.hip): k_dr with each subtree's CP families fused behind its forward
    // sweep, one launch per CP iteration (config 2: binary, 20 / 8, fp64, tiers of 4 levels, the
    // k_cp6 box patterns); RAOCP_DRC=0 keeps k_dr + k_cp6. Its residual rows alternate between two
    // sets of cp_rows rows (the extra workgroup tests the previous iteration beside the next)
    bool drc = false;
    raocp::DrcArg drca{};
    raocp::DrcArg* d_drca = nullptr;  // drca per iteration parity in device memory (k_drc reads it there)
    size_t drc_lds = 0;
    size_t dr_gran = 0;  // granules of each hand-off buffer
    double* x0 = nullptr;
    raocp::Bufs bufs{};          // {Z0, Z1, Z2, E0, E1}
    Ctl* ctl = nullptr;
    Ctl* h_ctl = nullptr;        // pinned host mirror
    raocp::CtlPub* h_pub = nullptr;  // pinned host memory the batch tail's stopping test publishes to
    raocp::CtlPub* d_pub = nullptr;  // (its device address)
    double* hist = nullptr;
    size_t hist_rows = 0;
    double* cur_z = nullptr;     // the Cache's current primal / dual
    double* cur_e = nullptr;
    double* tmpP = nullptr;      // staging for host-pointer calls
    double* tmpD = nullptr;
    double* part = nullptr;      // dot-product partials
    double* scal = nullptr;      // device scalars
    int cut = 0;                 // dynamics cut stage (0: per-stage kernels)
    raocp::Paths path{};         // what runs (raocp_path.h): resolve_ctx_paths, from the flags that say "was set up"
    double* redpart = nullptr;   // per-block residual maxima [red_rows][6]
    int red_rows = 0;
    size_t lds_top = 0;
    int dyn_block = 1024;        // tier workgroups (RAOCP_DYN_BLOCK)
    int dyn_top_block = 1024;    // the top's single workgroup (RAOCP_DYN_TOP_BLOCK)
    // node-block CP kernels (raocp_cp.hip): family / leaf block sizes, grid, LDS bytes
    int cp_FB = 1, cp_LB = 1, cp_nbF = 0, cp_nbL = 0;
    int ell_nb = 0, ell_threads = 512;  // L / L^T blocks (raocp_ell.hip), threads, LDS bytes
    size_t ell_lds = 0, ellt_lds = 0;
    size_t lds_cpd = 0, lds_cpp = 0;
    int cp_rows = 0;             // residual partial rows the CP iteration writes
    // MFMA CP kernels (raocp_cp2.hip): block shape, grid, LDS bytes; v1 = the scalar kernels
    int cp2_W = 4, cp2_FB = 1, cp2_LB = 16, cp2_nbF = 0, cp2_nbL = 0;
    size_t lds_cpd2 = 0, lds_cpp2 = 0;
    bool ell2_mixed = false;     // a node block of the MFMA kernels mixes weight tables: no k_ell2 / k_ellt2<float>
    bool cp_v1 = false;          // RAOCP_CP_V1=1: the scalar k_cpd / k_cpp (raocp_cp.hip)
    // host copies the CP tables are (re)built from (build_cp_blocks)
    std::vector<int> h_yrel, h_chs, h_nch, h_pos7, h_pos14;
    std::vector<int> h_isq, h_isr, h_isp;  // per-node weight table indices (uniform-table blocks)
    // subtree sharding (raocp_shard_setup): R shards own contiguous blocks of the
    // subtrees rooted at the top's boundary stage sh_S; the top is replicated
    int sh_R = 1, sh_r = 0, sh_S = 0;
    std::vector<int> own_lo, own_hi;                // per stage: owned id range
    std::vector<std::pair<int, int>> tier_own;      // per tier: {first subtree, count}
    int x_max = 0;                                  // largest slice of stage sh_S
    int own_first = 0, own_cnt = 0;                 // this shard's slice
    double *x2_send = nullptr, *x2_recv = nullptr;  // q rows of the roots
    double *x1_send = nullptr, *x1_recv = nullptr;  // (eta+, xi2) eta2 entries of the roots
    const int* d_slc = nullptr;                     // [2R] {first id, count} per shard
    double* red8 = nullptr;                         // this shard's maxima, then all-reduced
    void* comm = nullptr;                           // ncclComm_t when the transport is RCCL
    bool eager = false;                             // iterations launched without a graph
    int n_sq = 0, n_sr = 0, n_sp = 0, nbn = 1, nbl = 1;
    const int* ph = nullptr;     // dual placeholder offsets
    int n_ph = 0;
    bool has_x0 = false;
    std::vector<double> h_x0;
    bool no_defer_check = false; // RAOCP_DEFER_CHECK=0: k_cp_check after every iteration (defer_check)
                                 // (measured slower than its own launch: DESIGN.md)
    // captured CP iterations
    hipGraphExec_t graph = nullptr;      // kGraphBatch iterations (raocp_cp_run, raocp_cp_bench)
    int graph_iters = 0;
    hipGraphExec_t graph_rem = nullptr;  // the remainder batch of raocp_cp_bench (exactly K iterations)
    int prepared = 0;                    // raocp_cp_prepare(x0) set up a run of this many iterations
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int graph_rem_iters = 0;
    // batched solves (raocp_cp_batch_run): the slabs and the per-instance control of k_cpb
    // (raocp_cpb.hip), allocated once per batch size and history length and reused; a context
    // k_cpb does not cover keeps the results of its sequential solves on the host
    struct Batch {
        int B = 0;                   // instances of the last batch call (0: none yet)
        bool kernel = false;         // ... which k_cpb ran
        int cap_B = 0;               // instances the device buffers hold
        size_t hist_rows = 0;
        raocp::CpbSlab lay{};
        char* slab = nullptr;        // elements of the context's scalar type (wsz bytes each)
        Ctl* ctl = nullptr;
        int* done = nullptr;
        double* hist = nullptr;
        double* u0 = nullptr;
        // the Anderson acceleration of raocp_cp_batch_run_aa (k_cpa): a second slab per instance
        // and one log record per history row, sized for memory a_m and a_rows history rows
        bool accel = false;          // the last batch call was accelerated
        int a_m = 0;
        size_t a_rows = 0;
        size_t a_log_rows = 0;       // rows per instance the last accelerated batch's log is laid out by
        raocp::CpaSlab alay{};
        double* aslab = nullptr;
        double* alog = nullptr;
        std::vector<int> fk;         // final_k per instance
        std::vector<double> hz, he, hu0;  // the sequential solves' final iterates and first inputs
        std::vector<double> hx0;     // ... and the state each instance's last solve was solved from
    } bt;
    // evaluation of a primal (raocp_evaluate, raocp_eval.hip): the sweep's launch plan and one
    // device block [w (n) | val (n) | part (2 per workgroup of the node pass) | out (4) | x0 of a
    // stored primal (nx)], set up at the first evaluation
    std::vector<raocp::EvalLaunch> eval_plan;
    double* eval_buf = nullptr;
    int eval_grid = 0;
    // closed-loop simulation of a batch (raocp_cp_batch_mpc): the plant tables of the root's
    // children (host copies from create; A | B uploaded at the first simulation in the
    // context's scalar type) and the
    // device block of the per-step records, reused while it is large enough
    std::vector<double> h_mpc_ab, h_mpc_w;
    const double* d_mpc_ab = nullptr;
    void* mpc_buf = nullptr;
    size_t mpc_cap = 0;
    std::vector<void*> allocs;

    template <class T>
    int alloc(T** p, size_t count) {
        void* v = nullptr;
        if (count == 0) count = 1;
        hipError_t e = hipMalloc(&v, count * sizeof(T) + 64);  // slack: LDS-DMA reads whole 16-B chunks
        if (e != hipSuccess) return fail(RAOCP_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
        allocs.push_back(v);
        *p = (T*)v;
        return RAOCP_OK;
    }
    template <class T>
    int upload(const T** dst, const T* src, size_t count) {
        T* p = nullptr;
        int rc = alloc(&p, count);
        if (rc) return rc;
        if (count) HIPCHK(hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice));
        *dst = p;
        return RAOCP_OK;
    }
    template <class T>
    int upload_vec(const T** dst, const std::vector<T>& v) {
        return upload(dst, v.data(), v.size());
    }
};

namespace raocp {

// environment switches: each caller keeps its own default and combination rule
inline bool env_flag(const char* name, bool dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) != 0 : dflt;
}
inline int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
// RAOCP_FUSE_TIMEOUT_MS: how long a hand-off wait of the co-resident sweeps may last, in
// 100 MHz ticks (1000 ms by default: a wait normally lasts microseconds)
inline long long fuse_timeout_ticks() { return std::max(1, env_int("RAOCP_FUSE_TIMEOUT_MS", 1000)) * 100000LL; }

}  // namespace raocp

using raocp::env_flag;
using raocp::env_int;
using raocp::fuse_timeout_ticks;
