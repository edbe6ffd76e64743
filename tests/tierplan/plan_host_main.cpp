// The tier planner on the host (csrc/raocp_tierplan.h, no HIP dependency): regular trees built
// in memory (one class per stage, one kind and one pair per child slot), planned for 256 CUs, and
// the whole result compared with the plan the library picked before the planner became a function
// of its own (tests/test_tierplan_host.py says where the numbers come from). Prints every plan;
// exit status 1 when one differs.
#include "raocp_tierplan.h"

#include <cstdio>
#include <vector>

namespace {

struct Case {
    const char* name;
    int C, N;                // branching factor, last stage
    raocp::TierSizes z;      // nx, nu, KP, KF, NUP, PS, SKP, SKF, SNU as raocp_ctx_create lays them out
    bool fold_ok, per_stage;
    raocp::TierPlanResult want;
};

raocp::TierCut cut(int s0, int s1, int maxch, size_t lds_b, size_t lds_f, int fm, bool fold) {
    raocp::TierCut t;
    t.s0 = s0;
    t.s1 = s1;
    t.maxch = maxch;
    t.lds_b = lds_b;
    t.lds_f = lds_f;
    t.fm = fm;
    t.fold = fold;
    return t;
}
raocp::TierPlanResult plan(int cut_, size_t lds_top, int maxch_top, bool f_lds_top, bool fold_top,
                           std::vector<raocp::TierCut> tiers) {
    raocp::TierPlanResult r;
    r.cut = cut_;
    r.lds_top = lds_top;
    r.maxch_top = maxch_top;
    r.f_lds_top = f_lds_top;
    r.fold_top = fold_top;
    r.tiers = tiers;
    return r;
}

void print(const char* what, const raocp::TierPlanResult& r) {
    printf("  %s top{cut=%d, lds_top=%zu, maxch_top=%d, f_lds_top=%d, fold_top=%d}\n", what, r.cut, r.lds_top, r.maxch_top,
           (int)r.f_lds_top, (int)r.fold_top);
    for (const auto& t : r.tiers)
        printf("  %s tier{%d, %d, %d, %zu, %zu, %d, %d}\n", what, t.s0, t.s1, t.maxch, t.lds_b, t.lds_f, t.fm, (int)t.fold);
}

bool same(const raocp::TierPlanResult& a, const raocp::TierPlanResult& b) {
    if (a.cut != b.cut || a.lds_top != b.lds_top || a.maxch_top != b.maxch_top || a.f_lds_top != b.f_lds_top ||
        a.fold_top != b.fold_top || a.tiers.size() != b.tiers.size())
        return false;
    for (size_t k = 0; k < a.tiers.size(); ++k) {
        const raocp::TierCut &x = a.tiers[k], &y = b.tiers[k];
        if (x.s0 != y.s0 || x.s1 != y.s1 || x.maxch != y.maxch || x.lds_b != y.lds_b || x.lds_f != y.lds_f ||
            x.fm != y.fm || x.fold != y.fold)
            return false;
    }
    return true;
}

bool run(const Case& cs) {
    const int C = cs.C, N = cs.N;
    std::vector<int> stage_ptr(N + 2), cls_ptr(N + 1), pair_ptr(N + 1);
    int n = 0, cnt = 1;
    for (int s = 0; s <= N; ++s) {
        stage_ptr[s] = n;
        n += cnt;
        cnt *= C;
    }
    stage_ptr[N + 1] = n;
    const int m = stage_ptr[N];
    std::vector<int> ch_start(m), nch(m, C);
    for (int i = 0; i < m; ++i) ch_start[i] = 1 + C * i;
    for (int s = 0; s <= N; ++s) {
        cls_ptr[s] = s;       // one class per stage
        pair_ptr[s] = C * s;  // one pair per child slot of each class
    }
    const raocp::TierTree tr{n, N, stage_ptr.data(), ch_start.data(), nch.data(), cls_ptr.data(), pair_ptr.data(), C};
    // the argument structs' limits in raocp_common.h (kMaxLevels, kMaxTopStages); no tree here comes near them
    const raocp::TierLimits lim{31, 62};
    const raocp::TierPlanResult got = raocp::plan_tiers(tr, cs.z, lim, 256, cs.fold_ok, cs.per_stage);
    const bool ok = same(got, cs.want);
    printf("%s: C=%d N=%d n=%d nx=%d nu=%d: %s\n", cs.name, C, N, n, cs.z.nx, cs.z.nu, ok ? "ok" : "DIFFERS");
    print("got ", got);
    if (!ok) print("want", cs.want);
    return ok;
}

// Wide and ragged stage profiles (more than four children): no recorded plan, the property instead.
// Either the planner declines (cut = 0: the per-stage kernels) or the top [0, cut) and the tiers, the
// shallowest first, tile the parent stages [0, N) with no gap and no overlap, every tier non-empty,
// its widest level within the tree's widest stage, and every launch within the LDS budget.
// kids[s](q): the child count of the q-th node of stage s.
template <class Kids>
bool covers(const char* name, int N, const raocp::TierSizes& z, Kids kids) {
    std::vector<int> stage_ptr(N + 2), ch_start, nch, cls_ptr(N + 1), pair_ptr(N + 1);
    int n = 0, cnt = 1, cmax = 0, widest = 1;
    for (int s = 0; s <= N; ++s) {
        stage_ptr[s] = n;
        int next = 0;
        if (s < N)
            for (int q = 0; q < cnt; ++q) {
                const int c = kids(s, q);
                ch_start.push_back(n + cnt + next);
                nch.push_back(c);
                next += c;
                cmax = c > cmax ? c : cmax;
            }
        n += cnt;
        if (s < N) cnt = next;
        widest = cnt > widest ? cnt : widest;
    }
    stage_ptr[N + 1] = n;
    for (int s = 0; s <= N; ++s) {
        cls_ptr[s] = s;          // one class per stage
        pair_ptr[s] = cmax * s;  // one pair per child slot of each class
    }
    const raocp::TierTree tr{n, N, stage_ptr.data(), ch_start.data(), nch.data(), cls_ptr.data(), pair_ptr.data(), cmax};
    const raocp::TierLimits lim{31, 62};
    bool ok = true;
    for (int fold = 0; fold < 2; ++fold) {
        const raocp::TierPlanResult got = raocp::plan_tiers(tr, z, lim, 256, fold != 0, false);
        bool good = true;
        if (got.cut == 0) {
            good = got.tiers.empty();
        } else {
            int at = got.cut;
            good = got.cut >= 1 && got.cut <= N && got.lds_top <= raocp::kTierLds && got.maxch_top <= widest;
            for (const auto& t : got.tiers) {
                good = good && t.s0 == at && t.s1 > t.s0 && t.s1 <= N && t.maxch >= 1 && t.maxch <= widest &&
                       t.lds_b <= raocp::kTierLds + 2048 && t.lds_f <= raocp::kTierLds + 2048;
                at = t.s1;
            }
            good = good && at == N;
        }
        printf("%s fold_ok=%d: N=%d n=%d cmax=%d nx=%d nu=%d: %s\n", name, fold, N, n, cmax, z.nx, z.nu,
               good ? (got.cut ? "covers" : "declines") : "BROKEN");
        print("got ", got);
        ok = ok && good;
    }
    return ok;
}

}  // namespace

int main() {
    const raocp::TierSizes z20{20, 8, 24, 32, 8, 28, 26, 34, 10};
    const raocp::TierSizes z3{3, 2, 8, 8, 2, 6, 10, 10, 2};
    const raocp::TierSizes z64{64, 32, 64, 96, 32, 96, 66, 98, 34};
    const raocp::TierSizes z96{96, 48, 96, 144, 48, 144, 98, 146, 50};
    const std::vector<Case> cases{
        // config 2's tree
        {"bin12", 2, 12, z20, true, false,
         plan(4, 117200, 16, true, true, {cut(4, 8, 16, 63184, 54736, 1, true), cut(8, 12, 16, 63184, 54736, 1, true)})},
        {"bin12_nofold", 2, 12, z20, false, false,
         plan(4, 85840, 16, true, false, {cut(4, 8, 16, 31824, 54736, 1, false), cut(8, 12, 16, 31824, 54736, 1, false)})},
        // the "quad" tree of tests/test_gpu_dyn_split.py
        {"quad5", 4, 5, z20, true, false, plan(2, 103952, 16, true, true, {cut(2, 5, 64, 95952, 77328, 1, true)})},
        // the smallest tree that could hold a tier below the top: all of it goes into the top
        {"bin3_small", 2, 3, z3, true, false, plan(3, 6416, 8, true, true, {})},
        // F per level in the tiers (fm = 2), two-phase levels there, the top's F from global memory
        {"bin4_wide", 2, 4, z64, true, false,
         plan(1, 146992, 2, false, true, {cut(1, 2, 2, 129328, 118064, 1, true), cut(2, 4, 4, 161168, 136592, 2, false)})},
        // no top fits the LDS: per-stage kernels
        {"bin4_nofit", 2, 4, z96, true, false, plan(0, 0, 0, false, false, {})},
        // per-stage forced: the top's values are those of the plan it overrides
        {"bin12_per_stage", 2, 12, z20, true, true, plan(0, 117200, 16, true, true, {})},
    };
    int bad = 0;
    for (const Case& cs : cases) bad += run(cs) ? 0 : 1;
    printf("%d of %zu plans differ\n", bad, cases.size());
    const raocp::TierSizes z5{5, 3, 8, 8, 4, 10, 10, 10, 6}, z17{17, 5, 24, 24, 6, 24, 26, 26, 8};
    int broken = 0;
    broken += covers("five3", 3, z5, [](int, int) { return 5; }) ? 0 : 1;      // 156 nodes
    broken += covers("five6", 6, z20, [](int, int) { return 5; }) ? 0 : 1;     // 19,531 nodes: tiers below a top
    broken += covers("eight2", 2, z20, [](int, int) { return 8; }) ? 0 : 1;    // 73 nodes
    broken += covers("ragged2", 2, z17, [](int s, int q) { return s == 0 ? 12 : 1 + (7 * q) % 12; }) ? 0 : 1;  // 91 nodes
    broken += covers("ragged4", 4, z20, [](int s, int q) { return 1 + (7 * q + s) % 6; }) ? 0 : 1;
    broken += covers("root82", 2, z5, [](int s, int) { return s == 0 ? 82 : 2; }) ? 0 : 1;  // 247 nodes
    printf("%d of 6 wide profiles broken\n", broken);
    return bad || broken ? 1 : 0;
}
