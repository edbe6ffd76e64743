// The path rule on the host (csrc/raocp_path.h, no HIP dependency): resolve_paths against (a)
// named capability sets with the paths the library took for them before the rule became a
// function, written out here, and (b) every one of the 2^11 capability sets, unsharded and
// sharded, against the precedence chains of that library copied below as plain if cascades
// (tests/test_path_host.py says where they come from). Prints every named case and the number of
// mismatches; exit status 1 when there is one.
#include "raocp_path.h"

#include <cstdio>

using raocp::CpPath;
using raocp::DynPath;
using raocp::PathCaps;
using raocp::Paths;

namespace {

// ---- the record of the chains as they stood at the use sites. Not to be rewritten in terms of
// raocp_path.h: this is what resolve_paths is compared with.

// the flags and fields of raocp_ctx the chains read
struct Ctx {
    bool cp3, cp4, cp5, cp6, cp_v1, dr, drc, dyn2, dyn3, dyn_split;
    int cut, sh_S;
};

// launch_dynamics(c, ..., part = 0), then DynOp::run for what it dispatches to
DynPath chain_dyn(const Ctx* c) {
    const int part = 0;
    if (c->dr && c->sh_S == 0 && part == 0) {  // the regular-tree sweep (raocp_dynr.hip)
        return DynPath::Dr;
    }
    if (c->dyn3) {
        return DynPath::Dyn3;
    }
    if (c->dyn2) {
        return DynPath::Dyn2;
    }
    // DynOp::run
    const int s = c->cut;
    const bool sharded = c->sh_S > 0;
    if (s > 0 && c->dyn_split && !sharded && part == 0) {
        return DynPath::TiersSplit;
    }
    if (s > 0) {
        return DynPath::Tiers;
    }
    return DynPath::PerStage;
}

// enqueue_cp_iteration's kernels after the sweep: launch_cp3, or launch_cpd + launch_cpp
CpPath chain_cp(const Ctx* c) {
    if (c->cp3) {
        // launch_cp3
        if (c->cp6 && c->sh_S == 0) {
            return CpPath::Cp6;
        }
        if (c->cp5) {
            return CpPath::Cp5;
        }
        if (c->cp4 && c->sh_S == 0) {
            return CpPath::Cp4;
        }
        return CpPath::Cp3;
    } else {
        // launch_cpd / launch_cpp
        if (c->cp_v1) return CpPath::TwoLaunchV1;
        return CpPath::TwoLaunchMfma;
    }
}

// enqueue_cp_iteration's one-launch iteration (k_drc)
bool chain_fused(const Ctx* c) { return c->drc && c->sh_S == 0; }

// ---- named cases

const char* name(DynPath d) {
    switch (d) {
        case DynPath::PerStage: return "PerStage";
        case DynPath::Tiers: return "Tiers";
        case DynPath::TiersSplit: return "TiersSplit";
        case DynPath::Dyn2: return "Dyn2";
        case DynPath::Dyn3: return "Dyn3";
        case DynPath::Dr: return "Dr";
    }
    return "?";
}
const char* name(CpPath p) {
    switch (p) {
        case CpPath::TwoLaunchV1: return "TwoLaunchV1";
        case CpPath::TwoLaunchMfma: return "TwoLaunchMfma";
        case CpPath::Cp3: return "Cp3";
        case CpPath::Cp4: return "Cp4";
        case CpPath::Cp5: return "Cp5";
        case CpPath::Cp6: return "Cp6";
    }
    return "?";
}

enum : unsigned {
    kCp3 = 1u << 0, kCp4 = 1u << 1, kCp5 = 1u << 2, kCp6 = 1u << 3, kCpV1 = 1u << 4, kDr = 1u << 5, kDrc = 1u << 6,
    kDyn2 = 1u << 7, kDyn3 = 1u << 8, kDynSplit = 1u << 9, kTiers = 1u << 10, kAll = 1u << 11
};
PathCaps caps(unsigned m) {
    PathCaps k{};
    k.cp3 = m & kCp3;
    k.cp4 = m & kCp4;
    k.cp5 = m & kCp5;
    k.cp6 = m & kCp6;
    k.cp_v1 = m & kCpV1;
    k.dr = m & kDr;
    k.drc = m & kDrc;
    k.dyn2 = m & kDyn2;
    k.dyn3 = m & kDyn3;
    k.dyn_split = m & kDynSplit;
    k.tiers = m & kTiers;
    return k;
}
Ctx ctx(unsigned m, bool sharded) {
    // a cut at stage 3 of the plan and, on a shard, the same boundary stage (any positive values)
    return Ctx{(m & kCp3) != 0,  (m & kCp4) != 0,  (m & kCp5) != 0,      (m & kCp6) != 0,
               (m & kCpV1) != 0, (m & kDr) != 0,   (m & kDrc) != 0,      (m & kDyn2) != 0,
               (m & kDyn3) != 0, (m & kDynSplit) != 0, (m & kTiers) ? 3 : 0, sharded ? 3 : 0};
}

constexpr int kAny = -1;  // the table lists no value
struct Named {
    const char* what;
    unsigned mask;
    bool sharded;
    DynPath dyn;
    int cp;     // a CpPath, or kAny
    int fused;  // 0 / 1, or kAny
};
const Named kNamed[] = {
    {"cp3 cp6 dr drc tiers (config 2 default)", kCp3 | kCp6 | kDr | kDrc | kTiers, false, DynPath::Dr, (int)CpPath::Cp6, 1},
    {"cp3 cp6 dr drc tiers (config 2 default), sharded", kCp3 | kCp6 | kDr | kDrc | kTiers, true, DynPath::Tiers, (int)CpPath::Cp3, 0},
    {"cp3 cp6 dr tiers (RAOCP_DRC=0)", kCp3 | kCp6 | kDr | kTiers, false, DynPath::Dr, (int)CpPath::Cp6, 0},
    {"cp3 cp4 dr tiers (RAOCP_CP6=0)", kCp3 | kCp4 | kDr | kTiers, false, DynPath::Dr, (int)CpPath::Cp4, kAny},
    {"cp3 cp4 dr tiers (RAOCP_CP6=0), sharded", kCp3 | kCp4 | kDr | kTiers, true, DynPath::Tiers, (int)CpPath::Cp3, kAny},
    {"cp3 dr tiers", kCp3 | kDr | kTiers, false, DynPath::Dr, (int)CpPath::Cp3, kAny},
    {"cp3 cp5 dyn3 (configs 4, 5)", kCp3 | kCp5 | kDyn3, false, DynPath::Dyn3, (int)CpPath::Cp5, kAny},
    {"cp3 cp5 dyn3 (configs 4, 5), sharded", kCp3 | kCp5 | kDyn3, true, DynPath::Dyn3, (int)CpPath::Cp5, kAny},
    {"tiers dyn_split", kTiers | kDynSplit, false, DynPath::TiersSplit, (int)CpPath::TwoLaunchMfma, kAny},
    {"tiers dyn_split, sharded", kTiers | kDynSplit, true, DynPath::Tiers, (int)CpPath::TwoLaunchMfma, kAny},
    {"tiers cp_v1", kTiers | kCpV1, false, DynPath::Tiers, (int)CpPath::TwoLaunchV1, kAny},
    {"dyn2", kDyn2, false, DynPath::Dyn2, kAny, kAny},
    {"nothing", 0, false, DynPath::PerStage, (int)CpPath::TwoLaunchMfma, kAny},
};

}  // namespace

int main() {
    int bad = 0;
    for (const Named& n : kNamed) {
        const Paths p = raocp::resolve_paths(caps(n.mask), n.sharded);
        const bool ok = p.dyn == n.dyn && (n.cp == kAny || (int)p.cp == n.cp) && (n.fused == kAny || (int)p.fused == n.fused);
        printf("%-50s -> %s / %s / %s%s\n", n.what, name(p.dyn), name(p.cp), p.fused ? "fused" : "not fused",
               ok ? "" : "   DIFFERS from the recorded path");
        bad += !ok;
    }
    printf("%d of %d named cases differ\n", bad, (int)(sizeof(kNamed) / sizeof(kNamed[0])));

    int mismatches = 0, combos = 0;
    for (unsigned m = 0; m < kAll; ++m)
        for (int sh = 0; sh < 2; ++sh) {
            const Ctx c = ctx(m, sh != 0);
            const Paths p = raocp::resolve_paths(caps(m), sh != 0);
            ++combos;
            if (p.dyn != chain_dyn(&c) || p.cp != chain_cp(&c) || p.fused != chain_fused(&c)) {
                if (mismatches < 20)
                    printf("mismatch: caps 0x%03x %s: %s / %s / %d, the chains give %s / %s / %d\n", m,
                           sh ? "sharded" : "unsharded", name(p.dyn), name(p.cp), (int)p.fused, name(chain_dyn(&c)),
                           name(chain_cp(&c)), (int)chain_fused(&c));
                ++mismatches;
            }
        }
    printf("%d mismatches over %d combinations\n", mismatches, combos);
    return bad || mismatches ? 1 : 0;
}
