// raocp_eval_ops.h — the arithmetic of the evaluation (raocp_eval.hip) that a host program can
// run too: AVaR of a family's outcomes and the launch plan of the backward sweep. No HIP runtime
// dependency: a plain host compiler takes this file (tests/eval/avar_host_main.cpp).
#pragma once

#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RAOCP_EVAL_HD __host__ __device__ inline
#else
#define RAOCP_EVAL_HD inline
#endif

namespace raocp {

// threads of a workgroup of k_eval_sweep (one wave): one parent per thread
constexpr int kEvalSweepBlock = 64;

// AVaR_{alpha, p}(Z) = max of mu'Z over {alpha mu <= p, mu >= 0, 1'mu = 1} (risks.py:28-35) by
// the Rockafellar-Uryasev form: min over t in {Z_k} of t + (1 / alpha) sum_k p_k max(Z_k - t, 0)
// (the minimand is convex and piecewise linear in t with its kinks at the Z_k). No sort, no cap
// on c; continuous in Z, so ties between children cannot change the value. alpha = 0 is the
// plain maximum (no division); alpha = 1 comes out as the expectation. A NaN in Z gives NaN.
// P is the type the probabilities are held in (double, or float on an fp32 context); all
// arithmetic is double.
template <class ZP, class PP>
RAOCP_EVAL_HD double avar_ru(ZP Z, PP p, int c, double alpha) {
    double zmax = Z[0];
    for (int k = 1; k < c; ++k) {
        const double z = Z[k];
        zmax = (z > zmax || z != z) ? z : zmax;  // a NaN wins and stays (nothing compares above it)
    }
    if (zmax != zmax || !(alpha > 0.0)) return zmax;
    double best = zmax;  // t = max Z: the sum is empty
    for (int q = 0; q < c; ++q) {
        const double t = Z[q];
        double s = 0.0;
        for (int k = 0; k < c; ++k) {
            const double d = (double)Z[k] - t;
            if (d > 0.0) s += (double)p[k] * d;
        }
        const double v = s > 0.0 ? t + s / alpha : t;
        best = v < best ? v : best;
    }
    return best;
}

// One launch of k_eval_sweep: the parent stages s_hi, s_hi - 1, .., s_lo in that order. A launch
// of one stage (s_hi == s_lo) spreads its parents over `blocks` workgroups; the last launch
// (last = true, blocks = 1) runs the remaining top stages down to stage 0 in one workgroup with
// a barrier between two stages and writes the results.
struct EvalLaunch {
    int s_hi, s_lo;
    int blocks;
    bool last;
};

// The sweep's launches from stage_ptr (N + 2 entries: the first node id of stages 0 .. N, then
// n), deepest parent stage N - 1 first: one launch per stage while the stage has more parents
// than one workgroup takes, then one last launch of one workgroup for every stage above. Every
// parent stage 0 .. N - 1 is in exactly one launch.
inline std::vector<EvalLaunch> eval_sweep_plan(const std::vector<int>& stage_ptr, int block = kEvalSweepBlock) {
    std::vector<EvalLaunch> plan;
    const int N = (int)stage_ptr.size() - 2;
    if (N < 1 || block < 1) return plan;
    // the top: the longest run of stages 0 .. top whose parents all fit one workgroup (stage 0
    // is the root alone, so the run is never empty)
    int top = 0;
    while (top + 1 < N && stage_ptr[top + 2] - stage_ptr[top + 1] <= block) ++top;
    for (int t = N - 1; t > top; --t) {
        const int cnt = stage_ptr[t + 1] - stage_ptr[t];
        plan.push_back({t, t, (cnt + block - 1) / block, false});
    }
    plan.push_back({top, 0, 1, true});
    return plan;
}

}  // namespace raocp
