// raocp_tierplan.h — the tier plan of the tiered dynamics sweep (raocp_dyn.hip / raocp_dynf.hip)
// as a pure host function: no HIP include and no raocp_ctx, so tests/tierplan/plan_host_main.cpp
// builds it with the host compiler alone. raocp_capi.hip (raocp_setup.h, plan_tiers and
// build_tier_plans) turns the result into launches.
//
// The stages are split into tiers 0 = s_0 < s_1 < ... < s_T = N:
// tier 0 (stages < s_1) runs backward + forward in ONE workgroup (k_dyn_top); every
// deeper tier [s_k, s_k+1) runs one workgroup per subtree rooted at stage s_k
// (k_dyn_bottom_back / _fwd), its boundary being the leaves or the next tier's roots.
// Vectors and matrix tables live in LDS (F when it fits). The cut list minimises a
// cost model: a level costs one unit per phase plus its lane work over 384, a tier
// kernel five units of launch + prologue. Per-stage launches when nothing fits (cut = 0).
#pragma once

#include <algorithm>
#include <cstddef>
#include <vector>

namespace raocp {

// read-only view of the tree: stage_ptr [N + 2], ch_start / nch [nonleaf nodes], cls_ptr
// [N + 1] (first class of each stage), pair_ptr [classes + 1] (first pair of each class)
struct TierTree {
    int n, N;
    const int* stage_ptr;
    const int* ch_start;
    const int* nch;
    const int* cls_ptr;
    const int* pair_ptr;
    int nkind;
};
// the padded row sizes and table row strides of the sweep (raocp_dyn.hip header)
struct TierSizes {
    int nx, nu;
    int KP, KF, NUP, PS;
    int SKP, SKF, SNU;
};
// limits of the kernels' argument structs (raocp_common.h kMaxLevels, kMaxTopStages)
struct TierLimits {
    int max_levels, max_top_stages;
};
// doubles of one table of each kind: W / WT, RG, K, F
struct TierTabs {
    size_t W1, RG1, KM1, F1;
};
inline TierTabs tier_tabs(const TierSizes& z) {
    const int R = z.nx + z.nu;
    return TierTabs{(size_t)R * z.SKP, (size_t)R * z.SNU, (size_t)z.nu * z.SKP, (size_t)z.nx * z.SKF};
}
constexpr size_t kTierLds = 160 * 1024 - 2 * 1024;  // minus the static LDS (Prologue, ~1.2 KB)
inline size_t tier_recs(size_t cnt) { return 2 * cnt; }  // 16-B records in doubles

struct TierCut {  // a tier [s0, s1) below the top
    int s0 = 0, s1 = 0, maxch = 0;
    size_t lds_b = 0, lds_f = 0;
    int fm = 1;         // F in the forward kernel: 0 global, 1 LDS, 2 LDS per level
    bool fold = false;  // one-phase backward levels (WT tables)
};
struct TierPlanResult {
    int cut = 0;  // the top's stages [0, cut); 0: per-stage kernels
    size_t lds_top = 0;
    int maxch_top = 0;
    bool f_lds_top = false, fold_top = false;
    std::vector<TierCut> tiers;  // the tiers below the top, the shallowest first
};

// fold_ok: one-phase backward levels allowed (per-pair WT tables instead of per-kind W, no P
// rows); per_stage: the per-stage kernels forced (cut = 0; the top's values are still reported)
inline TierPlanResult plan_tiers(const TierTree& tr, const TierSizes& z, const TierLimits& lim, int n_cus, bool fold_ok,
                                 bool per_stage) {
    const int N = tr.N, nx = z.nx, nu = z.nu, R = nx + nu;
    const int KP = z.KP, KF = z.KF, NUP = z.NUP, PS = z.PS, nkind = tr.nkind;
    const size_t kLds = kTierLds;
    const TierTabs tb_ = tier_tabs(z);
    const size_t W1 = tb_.W1, RG1 = tb_.RG1, KM1 = tb_.KM1, F1 = tb_.F1;
    const int* cp = tr.cls_ptr;
    const int* pp = tr.pair_ptr;
    const int* stage_ptr = tr.stage_ptr;
    auto stage_n = [&](int st) { return stage_ptr[st + 1] - stage_ptr[st]; };
    auto rup2 = [](int a) { return (a + 1) / 2 * 2; };
    auto recs = [](size_t cnt) { return tier_recs(cnt); };
    const long wg_per_cu = 2;
    auto level_cost = [&](double P, double C) { return 3.0 + (C * R + P * R + P * nu + C * nx) / 384.0; };
    auto top_bytes = [&](int s_, int& maxch, bool fl, bool fold) {
        const size_t T = stage_ptr[s_], nb = stage_n(s_);
        maxch = 0;
        for (int st = 1; st <= s_; ++st) maxch = std::max(maxch, stage_n(st));
        const size_t mats = (fold ? pp[cp[s_]] * W1 : nkind * W1) + cp[s_] * (RG1 + KM1) + (fl ? pp[cp[s_]] * F1 : 0);
        const size_t dbl = mats + T * KP + nb * KP + T * NUP + T * KF + (fold ? 0 : rup2(maxch * PS)) +
                           recs(T + T + nb - 1);
        return 8 * dbl;
    };
    struct Tier {
        size_t nall = 0, nnl = 0;
        int maxch = 0;
        double cost = 0;
        size_t bb = 0, bf = 0;
        int fm = 1;
        bool ok = false, fold = false;
    };
    auto tier = [&](int a, int b) {  // subtrees rooted at stage a, levels a..b-1, boundary b (worst case)
        Tier w;
        if (b - a > lim.max_levels) return w;
        std::vector<double> lvl(b - a, 0.0);
        for (int r = stage_ptr[a]; r < stage_ptr[a + 1]; ++r) {
            int lo = r, hi = r + 1, mc = 0;
            size_t nall = 0;
            for (int st = a; st < b; ++st) {
                nall += hi - lo;
                const int nlo = tr.ch_start[lo], nhi = tr.ch_start[hi - 1] + tr.nch[hi - 1];
                lvl[st - a] = std::max(lvl[st - a], level_cost(hi - lo, nhi - nlo));
                mc = std::max(mc, nhi - nlo);
                lo = nlo;
                hi = nhi;
            }
            w.nnl = std::max(w.nnl, nall);
            w.nall = std::max(w.nall, nall + (hi - lo));
            w.maxch = std::max(w.maxch, mc);
        }
        for (double v : lvl) w.cost += v;
        const size_t ncl = cp[b] - cp[a], npr = pp[cp[b]] - pp[cp[a]];
        w.bb = 8 * (nkind * W1 + ncl * RG1 + w.nall * KP + w.nnl * NUP + rup2(w.maxch * PS) + recs(w.nnl + w.nall - 1));
        const size_t bb_fold = 8 * (npr * W1 + ncl * RG1 + w.nall * KP + w.nnl * NUP + recs(w.nnl + w.nall - 1));
        if (fold_ok && bb_fold <= kLds) {
            w.fold = true;
            w.bb = bb_fold;
            w.cost -= (b - a);  // one barrier phase per backward level instead of two
        }
        w.bf = 8 * (ncl * KM1 + npr * F1 + w.nnl * KF + recs(w.nnl + w.nall - 1));
        if (w.bf > kLds) {
            // the pairs of one level at a time (restaged per level: one LDS round trip each),
            // else F from L2: measured 86.7 us for the config-4 tier [6,10) forward, whose
            // leaf level alone took 18.7 us per round (profiles/r03_v2/stamps_c4.log)
            size_t npl = 0;
            for (int t = a; t < b; ++t) npl = std::max<size_t>(npl, pp[cp[t + 1]] - pp[cp[t]]);
            const size_t bf2 = w.bf - 8 * (npr - npl) * F1;
            if (bf2 <= kLds) {
                w.fm = 2;
                w.bf = bf2;
                w.cost += (b - a - 1);
            } else {
                w.fm = 0;
                w.bf -= 8 * npr * F1;
                w.cost += 8 * (b - a);
            }
        }
        // the tier's subtrees run as rounds of co-resident workgroups (2048 lanes per CU
        // at most, fewer workgroups when their LDS does not fit): every round
        // pays the levels again (measured at configs 3 / 4: deep tiers of thousands of
        // subtrees lost to one-level tiers)
        {
            const size_t lds = std::max(w.bb, w.bf);
            const long per_cu = std::max<long>(1, std::min<long>(wg_per_cu, lds ? (long)(160 * 1024 / lds) : wg_per_cu));
            const long nsub = stage_ptr[a + 1] - stage_ptr[a];
            const long rounds = (nsub + (long)n_cus * per_cu - 1) / ((long)n_cus * per_cu);
            w.cost *= (double)std::max<long>(1, rounds);
        }
        w.cost += 10.0;  // two launches and their prologues
        w.ok = w.bb <= kLds && w.bf <= kLds;
        return w;
    };
    // f[a]: best cost of tiers covering [a, N); nxt[a]: the end of the first of them, first[a]: that tier
    std::vector<double> f(N + 1, 1e300);
    std::vector<int> nxt(N + 1, N);
    std::vector<Tier> first(N + 1);
    f[N] = 0.0;
    for (int a = N - 1; a >= 1; --a)
        for (int b = a + 1; b <= N; ++b) {
            if (f[b] >= 1e299) continue;
            const Tier w = tier(a, b);
            if (!w.ok) continue;
            if (w.cost + f[b] < f[a]) {
                f[a] = w.cost + f[b];
                nxt[a] = b;
                first[a] = w;
            }
        }
    TierPlanResult res;
    double best = 1e300;
    int best_s = 0;
    double top_cost = 5.0;
    for (int s_ = 1; s_ <= N && s_ <= lim.max_top_stages; ++s_) {
        top_cost += level_cost(stage_n(s_ - 1), stage_n(s_));
        bool any = false;
        for (int v = 0; v < 4; ++v) {  // (F in LDS, fold) = (1,1), (1,0), (0,1), (0,0)
            const bool fl = v < 2, fold = (v % 2 == 0);
            if (fold && !fold_ok) continue;
            int mt = 0;
            const size_t tb = top_bytes(s_, mt, fl, fold);
            if (tb > kLds) continue;
            any = true;
            const double cost = top_cost + (fl ? 0.0 : 2.0 * s_) - (fold ? s_ : 0) + f[s_];
            if (cost < best) {
                best = cost;
                best_s = s_;
                res.lds_top = tb;
                res.maxch_top = mt;
                res.f_lds_top = fl;
                res.fold_top = fold;
            }
        }
        if (!any) break;
    }
    res.cut = best_s;
    if (per_stage) res.cut = 0;
    if (res.cut > 0 && f[res.cut] >= 1e299) res.cut = 0;
    for (int a = res.cut; res.cut > 0 && a < N; a = nxt[a]) {
        const Tier& w = first[a];
        TierCut tc;
        tc.s0 = a;
        tc.s1 = nxt[a];
        tc.maxch = w.maxch;
        tc.lds_b = w.bb;
        tc.lds_f = w.bf;
        tc.fm = w.fm;
        tc.fold = w.fold;
        res.tiers.push_back(tc);
    }
    return res;
}

}  // namespace raocp
