// raocp_eval.h — host interface of raocp_eval.hip: the evaluation of a primal (the nested-AVaR
// cost of its policy, the epigraph value, the box violation and the dynamics residual).
#pragma once

#include <string>
#include <vector>

#include "raocp_common.h"
#include "raocp_cpb_layout.h"
#include "raocp_eval_ops.h"

namespace raocp {

constexpr int kEvalBlock = 256;            // threads of a workgroup of k_eval_nodes / k_eval_batch
constexpr int kEvalMaxGrid = 2048;         // workgroups of k_eval_nodes at most (8 per CU)
constexpr int kEvalBatchLdsW = 48 * 1024;  // LDS budget of k_eval_batch's per-node work array (bytes)

// The kernels are templates on the context's scalar type T (double, or float on an fp32
// context): the primal, x0 and Dev's L weights, box bounds, alpha_r and cond hold T. The dynamics
// table dW ([B'; A'] per child kind, rows of w_stride doubles) is fp64 on a context of either
// precision. Every value is widened at its load; all arithmetic and every output is double.
struct EvalArg {
    const void* z;    // T [P] the primal (device)
    const void* x0;   // T [nx] the initial state
    double* w;        // [n] l_j + V_j (node 0: V_0)
    double* val;      // [n] V_j
    double* part;     // [grid][2] per workgroup of k_eval_nodes: box violation, dynamics residual
    double* out;      // [4] RAOCP_EVAL_COST .. RAOCP_EVAL_DYN
    int grid;         // workgroups of k_eval_nodes
    int w_stride;     // doubles per row of dW
};

// workgroups of k_eval_nodes for this tree (its nodes spread over groups of lanes; at most
// kEvalMaxGrid, a workgroup then loops)
int eval_nodes_grid(const Dev& p);
// k_eval_nodes, then the sweep's launches in plan order, on one stream
hipError_t eval_launch(const Dev& p, const EvalArg& a, const std::vector<EvalLaunch>& plan, bool f32,
                       hipStream_t stream);
// "k_eval_nodes<double> + k_eval_sweep<double> xS"
std::string eval_name(bool f32, int sweeps);

// k_eval_batch: one workgroup per instance of a batch, over the instance's final primal inside
// its slab (CpbSlab offsets in elements of T), x0 the slab's own initial state
struct EvalBatchArg {
    const void* slab;
    CpbSlab lay;
    const int* zsel;  // [B] which of the three primals of the slab is the final one
    double* out;      // [B][4]
    double* scratch;  // [B][n] the work arrays when they do not fit LDS (else unused)
    int B;
    int w_stride;
};
// true when the per-node work array of one instance (n doubles) fits kEvalBatchLdsW
bool eval_batch_w_in_lds(const Dev& p);
hipError_t eval_batch_launch(const Dev& p, const EvalBatchArg& a, bool f32, hipStream_t stream);
const char* eval_batch_name(bool f32);

}  // namespace raocp
