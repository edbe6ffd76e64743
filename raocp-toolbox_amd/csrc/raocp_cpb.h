// raocp_cpb.h — host interface of raocp_cpb.hip: the batched Chambolle–Pock kernel k_cpb
// (one workgroup per instance of a batch that shares the tree, the tables and alpha and
// differs in x0 and, optionally, in the starting iterate).
#pragma once

#include "raocp_common.h"

namespace raocp {

constexpr int kCpbBlock = 256;        // threads per workgroup (one instance)
constexpr int kCpbMaxNx = 32;         // runtime sizes the kernel covers
constexpr int kCpbMaxNu = 16;
constexpr int kCpbLdsTabs = 32 * 1024;  // LDS budget of the staged tables (bytes): >= 4 workgroups per CU

// one instance's slab in HBM: offsets in doubles from the slab's start, every array on a 16-B
// boundary, `stride` doubles (a multiple of 32: 256 B) between the slabs of two instances
struct CpbSlab {
    long z[3];    // the rotating primals (P each)
    long e[2];    // the rotating duals (D each)
    long xi2;     // xi2 (D)
    long tv;      // the dual half step v before its projection (D)
    long q;       // q rows of the dynamics projection (n x nx)
    long dd;      // d rows (m x nu)
    long pb;      // child products [h | a] (n x (nu + nx))
    long x0;      // the instance's initial state (nx)
    long stride;
};

struct CpbArg {
    double* slab;      // [B] slabs
    CpbSlab lay;
    Ctl* ctl;          // [B] control blocks (pad: 1 once the first half step is done)
    int* done;         // [B] the done words the host polls
    double* hist;      // [B][hist_rows][6]
    long hist_rows;
    double* u0;        // [B][nu] the root's input of the final iterate
    int B;
    int chunk;         // CP iterations per launch
    int lds_tabs;      // the L weights and the box tables are staged in LDS
};

// k_mpc_step: the end of one closed-loop MPC step of a batch and the start of the next, inside
// the slabs (after every instance of the batch is done with step t)
struct MpcArg {
    const double* ab;    // [nch[0]] {A_i (nx x nx) | B_i (nx x nu)} row-major, i = ch_start[0] + j
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

CpbSlab cpb_layout(const Dev& p);
// bytes of LDS the staged tables take, 0 when they exceed kCpbLdsTabs (then read from HBM)
size_t cpb_tab_bytes(const Dev& p);
hipError_t cpb_launch(const Dev& p, const CpbArg& a, hipStream_t stream);
const char* cpb_name(bool lds_tabs);
hipError_t mpc_step_launch(const Dev& p, const CpbArg& a, const MpcArg& m, hipStream_t stream);
const char* mpc_step_name();

}  // namespace raocp
