// raocp_cpb.h — host interface of raocp_cpb.hip: the batched Chambolle–Pock kernel k_cpb
// (one workgroup per instance of a batch that shares the tree, the tables and alpha and
// differs in x0 and, optionally, in the starting iterate).
#pragma once

#include "raocp_common.h"
#include "raocp_cpb_layout.h"
#include "raocp_cpa_layout.h"
#include "raocp_aa_ops.h"

namespace raocp {

constexpr int kCpbBlock = 256;        // threads per workgroup (one instance)
constexpr int kCpbMaxNx = 32;         // runtime sizes the kernel covers
constexpr int kCpbMaxNu = 16;
constexpr int kCpbLdsTabs = 32 * 1024;  // LDS budget of the staged tables (bytes): >= 4 workgroups per CU

// The kernels are templates on the context's scalar type T (double, or float on an fp32
// context): the slabs, the shared tables and the root-children table of MpcArg hold T; the
// control blocks, the history rows, u0 and the records of MpcArg are double / int for either T.
struct CpbArg {
    void* slab;        // [B] slabs of T (CpbSlab offsets are in elements of T)
    CpbSlab lay;
    Ctl* ctl;          // [B] control blocks (pad: 1 once the first half step is done)
    int* done;         // [B] the done words the host polls
    double* hist;      // [B][hist_rows][6]
    long hist_rows;
    double* u0;        // [B][nu] the root's input of the final iterate
    int B;
    int chunk;         // CP iterations per launch
    int lds_tabs;      // the L weights and the box tables are staged in LDS
    // T = float only: the dynamics tables as an fp32 context holds them (the column-major
    // M[k rows + r] tables of its per-stage dynamics: W, RG, K, F; Dev's dW .. dF are fp64)
    const void* W2;
    const void* RG2;
    const void* KM2;
    const void* F2;
};

// k_mpc_step: the end of one closed-loop MPC step of a batch and the start of the next, inside
// the slabs (after every instance of the batch is done with step t)
struct MpcArg {
    const void* ab;      // T [nch[0]] {A_i (nx x nx) | B_i (nx x nu)} row-major, i = ch_start[0] + j
    const int* scen;     // [B][T] realised root child j of instance b at step t
    int* frz;            // [B] the step at which the instance froze (NaN in a box), -1: running
    double* X;           // [B][T + 1][nx]
    double* U;           // [B][T][nu]
    double* cost;        // [B][T]
    int* status;         // [B][T]
    int* iters;          // [B][T]
    double* err;         // [B][T][3]
    int T;
    int t;               // the step that ends
    int warm;            // the next solve starts from this step's final iterate (else from zero)
    int last;            // t == T - 1: record only, the slab keeps the last solve
};

// k_cpa: k_cpb's iteration with Anderson acceleration (fp64 only). The CP iterate stays in the
// CpbSlab of CpbArg; the acceleration's history and state live in a second slab per instance.
struct CpaArg {
    double* slab;        // [B] CpaSlab
    CpaSlab lay;
    double* log;         // [B][hist_rows][kAaRec] one record per iteration
    int every;           // a proposal after iteration k when (k + 1) % every == 0
    double reg;          // relative Tikhonov term of the normal equations
    double safeguard;    // a trial is accepted when |T(v^) - v^|_2 <= safeguard |r_k|_2
};
CpaSlab cpa_layout(const Dev& p, int m);
hipError_t cpa_launch(const Dev& p, const CpbArg& a, const CpaArg& aa, hipStream_t stream);
const char* cpa_name(bool lds_tabs);

// f32: the context's scalar type is float (its Dev tables hold floats)
CpbSlab cpb_layout(const Dev& p, bool f32);
// bytes of LDS the staged tables take in the context's type, 0 when they exceed kCpbLdsTabs
// (then read from HBM)
size_t cpb_tab_bytes(const Dev& p, bool f32);
hipError_t cpb_launch(const Dev& p, const CpbArg& a, bool f32, hipStream_t stream);
// the names raocp_kernel_info reports: the fp64 forms keep the strings they had before the
// kernels took a type ("k_cpb<true>", "k_mpc_step"), the fp32 forms name it
const char* cpb_name(bool f32, bool lds_tabs);
hipError_t mpc_step_launch(const Dev& p, const CpbArg& a, const MpcArg& m, bool f32, hipStream_t stream);
const char* mpc_step_name(bool f32);
// k_mpc_step_aa: k_mpc_step after a step that k_cpa solved (fp64 only). It also reduces the
// instance's log rows 0 .. final_k to counts[b][t][kAaCounts] and, unless the step is the last,
// leaves the instance's CpaState and G as the memset of a fresh accelerated batch does.
hipError_t mpc_step_aa_launch(const Dev& p, const CpbArg& a, const MpcArg& m, const CpaArg& aa, int* counts,
                              hipStream_t stream);
const char* mpc_step_aa_name();

}  // namespace raocp
