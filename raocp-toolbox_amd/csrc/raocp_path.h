// raocp_path.h — which kernels a context runs, resolved once from what was set up: a pure host
// function (no HIP include and no raocp_ctx), so tests/path/path_host_main.cpp builds it with the
// host compiler alone. raocp_capi.hip stores the result in raocp_ctx::path (resolve_ctx_paths, at
// the end of raocp_ctx_create and again at the end of raocp_shard_setup) and every launch, name
// and error-word site switches on it.
//
// A capability says that a form was set up (its tables, task lists and grids exist); a shard
// (raocp_shard_setup) runs none of the forms that span the whole tree: k_dr, k_drc, k_cp6, k_cp4
// and the split tier sweep.
#pragma once

namespace raocp {

// the dynamics projection
enum class DynPath {
    PerStage,    // k_dyn_gather + k_dyn_stage_a / _b / _f (raocp_dyn.hip)
    Tiers,       // k_dyn_bottom_back, k_dyn_top, k_dyn_bottom_fwd (raocp_dyn.hip)
    TiersSplit,  // k_dyn_up + k_dyn_down (raocp_dynf.hip)
    Dyn2,        // the per-stage MFMA kernels (raocp_dyn2.hip)
    Dyn3,        // the per-stage streaming sweep (raocp_dyn3.hip)
    Dr           // the regular-tree sweep (raocp_dynr.hip)
};
// the CP kernels after the projection
enum class CpPath {
    TwoLaunchV1,    // k_cpd + k_cpp (raocp_cp.hip)
    TwoLaunchMfma,  // k_cpd2 + k_cpp2 (raocp_cp2.hip)
    Cp3,            // from here on the fused forms (cp_fused): k_cp3 (raocp_cp3.hip)
    Cp4,            // k_cp4 (raocp_cp4.hip)
    Cp5,            // k_cp5_leaf + k_cp5_fam (raocp_cp5.hip)
    Cp6             // k_cp6 (raocp_cp5.hip)
};
struct PathCaps {  // (resolve_ctx_paths fills it positionally: keep the order)
    bool cp3, cp4, cp5, cp6, cp_v1, dr, drc, dyn2, dyn3, dyn_split;
    bool tiers;  // the tier plan has a cut (raocp_ctx::cut > 0)
};
struct Paths {
    DynPath dyn;
    CpPath cp;
    bool fused;  // k_drc: projection and CP iteration in one launch (set up only beside Dr and Cp6)
};

inline bool cp_fused(CpPath p) { return p >= CpPath::Cp3; }

inline Paths resolve_paths(const PathCaps& k, bool sharded) {
    Paths p{};
    p.dyn = k.dr && !sharded                        ? DynPath::Dr
            : k.dyn3                                ? DynPath::Dyn3
            : k.dyn2                                ? DynPath::Dyn2
            : k.tiers && k.dyn_split && !sharded    ? DynPath::TiersSplit
            : k.tiers                               ? DynPath::Tiers
                                                    : DynPath::PerStage;
    if (!k.cp3) p.cp = k.cp_v1 ? CpPath::TwoLaunchV1 : CpPath::TwoLaunchMfma;
    else
        p.cp = k.cp6 && !sharded   ? CpPath::Cp6
               : k.cp5             ? CpPath::Cp5
               : k.cp4 && !sharded ? CpPath::Cp4
                                   : CpPath::Cp3;
    p.fused = k.drc && !sharded;
    return p;
}

}  // namespace raocp
