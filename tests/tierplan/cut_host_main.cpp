// The top's cut of a tree's tier plan on the host (csrc/raocp_tierplan.h, no HIP dependency), for
// tests/branch_cases.py: the stage raocp_shard_setup cuts a tiered-sweep context at is c->cut, the
// planner's choice. Reads the tree as raocp_ctx_create hands it to the planner from standard input
// (whitespace-separated integers):
//   N n nkind nx nu n_cus, stage_ptr [N + 2], m, ch_start [m], nch [m], cls_ptr [N + 1], nk,
//   pair_ptr [nk + 1]
// and prints "cut <S>" and one "tier <s0> <s1>" line per tier below the top. The padded sizes are
// those of raocp_setup.h (KP, KF: nx, nx + nu rounded up to 8; NUP: nu to 2; PS = NUP + nx to 2;
// the table strides by raocp_dyn.hip's tstride); fold allowed, per-stage not forced (the defaults).
#include "raocp_tierplan.h"

#include <cstdio>
#include <vector>

namespace {
int rup(int a, int b) { return (a + b - 1) / b * b; }
int tstride(int k) { return (k / 2) % 2 == 0 ? k + 2 : k; }
bool read(std::vector<int>& v, int cnt) {
    v.resize(cnt);
    for (int& x : v)
        if (scanf("%d", &x) != 1) return false;
    return true;
}
}  // namespace

int main() {
    int N, n, nkind, nx, nu, n_cus, m, nk;
    if (scanf("%d %d %d %d %d %d", &N, &n, &nkind, &nx, &nu, &n_cus) != 6 || N < 1 || n < 2) return 2;
    std::vector<int> stage_ptr, ch_start, nch, cls_ptr, pair_ptr;
    if (!read(stage_ptr, N + 2) || scanf("%d", &m) != 1 || m < 1 || !read(ch_start, m) || !read(nch, m) ||
        !read(cls_ptr, N + 1) || scanf("%d", &nk) != 1 || nk < 1 || !read(pair_ptr, nk + 1))
        return 2;
    const int KP = rup(nx, 8), KF = rup(nx + nu, 8), NUP = rup(nu, 2), PS = NUP + rup(nx, 2);
    const raocp::TierSizes z{nx, nu, KP, KF, NUP, PS, tstride(KP), tstride(KF), tstride(NUP)};
    const raocp::TierTree tr{n, N, stage_ptr.data(), ch_start.data(), nch.data(), cls_ptr.data(), pair_ptr.data(), nkind};
    // the argument structs' limits in raocp_common.h (kMaxLevels, kMaxTopStages), as plan_host_main.cpp
    const raocp::TierPlanResult res = raocp::plan_tiers(tr, z, raocp::TierLimits{31, 62}, n_cus, true, false);
    printf("cut %d\n", res.cut);
    for (const auto& t : res.tiers) printf("tier %d %d\n", t.s0, t.s1);
    return 0;
}
