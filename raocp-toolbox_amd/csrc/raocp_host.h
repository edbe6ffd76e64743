// raocp_host.h -- what the host units of the library (raocp_capi.hip, raocp_batch.hip) share
// beside the context (raocp_ctx.h): the guards every entry point opens with, an owning pointer
// for temporary device memory, and the functions one unit defines and the other calls.
#pragma once

#include <mutex>

#include "raocp_ctx.h"

namespace raocp {

// Every entry point that takes a context runs on that context's device: the current
// device is switched for the call and restored afterwards (a process may hold contexts
// on several devices; allocations and graph captures must land on c->device).
// The co-resident sweeps (k_dr, k_drc and the split tier sweep k_dyn_up / k_dyn_down) spin on
// hand-off flags and need every workgroup of their launch resident at once. Two of them from
// different contexts on one device could each hold part of the CUs and wait for the other
// (until the hand-off timeout returns RAOCP_ERR_STATE). One active context per device: the entry
// points that launch them hold a per-device lock for the call (each synchronises its stream
// before it returns), so threads of one process run such contexts one at a time. Processes
// sharing a device are not serialised (docs: INTEGRATION.md "one active context per device").
inline std::recursive_mutex g_sweep_mu[64];  // (inline: one array in the library, whichever unit locks)
struct SweepLock {
    std::unique_lock<std::recursive_mutex> l;
    explicit SweepLock(const raocp_ctx* c) {
        if (c && (c->dr || c->dyn_split)) l = std::unique_lock<std::recursive_mutex>(g_sweep_mu[c->device & 63]);
    }
};

struct DevGuard {
    int prev = -1;
    explicit DevGuard(const raocp_ctx* c) {
        if (!c) return;
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != c->device) (void)hipSetDevice(c->device);
        else prev = -1;
    }
    ~DevGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// temporary device memory, freed when it leaves scope
struct DevMem {
    void* p = nullptr;
    DevMem() = default;
    DevMem(DevMem&& o) noexcept : p(o.p) { o.p = nullptr; }
    DevMem(const DevMem&) = delete;
    DevMem& operator=(const DevMem&) = delete;
    ~DevMem() {
        if (p) (void)hipFree(p);
    }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
};

// raocp_capi.hip: host fp64 arrays <-> the context's device vectors, and a table uploaded as
// the context's scalar type
int copy_in(raocp_ctx* c, double* dst, const double* src, size_t count, int flags);
int copy_out(raocp_ctx* c, double* dst, const double* src, size_t count, int flags);
int upload_t(raocp_ctx* c, const double** dst, const std::vector<double>& v);

// raocp_batch.hip: whether k_cpb covers the context's batched solves (kernel_name), the release
// of the batch and MPC buffers (raocp_ctx_destroy), and the evaluation's buffers and kernel
// arguments (raocp_op_bench op 17)
bool cpb_on(const raocp_ctx* c);
void batch_free(raocp_ctx* c);
void mpc_free(raocp_ctx* c);
int eval_ensure(raocp_ctx* c);
EvalArg eval_arg(raocp_ctx* c, const void* dz, const void* dx0);

}  // namespace raocp

using raocp::DevGuard;
using raocp::DevMem;
using raocp::SweepLock;
using raocp::batch_free;
using raocp::copy_in;
using raocp::copy_out;
using raocp::cpb_on;
using raocp::eval_arg;
using raocp::eval_ensure;
using raocp::mpc_free;
using raocp::upload_t;
