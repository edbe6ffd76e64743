// raocp_setup.h -- how a context is built: the stages raocp_ctx_create runs in order, each a
// file-local function returning an error code, with the helpers they share (the CP block
// tables, the regular-tree sweep's and k_drc's setup). Included by raocp_capi.hip only, after
// the launch wrappers the stages use.
#pragma once

#include "raocp_tierplan.h"

namespace {

// host tables of the flat layout that later stages read
struct Layout {
    std::vector<int> yrel, e7off, e14off, rank, ph;
};

// the dynamics tables on the host (raocp_dyn.hip header): per node its child kind and (kind,
// parent class) pair, the kinds and pairs, per child kind W = [B'; A'], per class
// RG = [R~^-1; G = M R~^-1 - K'] and K, per pair F = [A + B K | B] and WT; rows padded to the
// strides SKP / SKF / SNU
struct DynTables {
    std::vector<int> kind, pair;
    std::vector<std::pair<int, int>> kinds, pairs;
    std::vector<double> W, RG, KM, F, WT;
    int SKP = 0, SKF = 0, SNU = 0, R = 0;
};

// the residual partials [red_rows][6] hold at least `rows` rows: a larger block is allocated
// and zeroed when they do not (the old one stays in c->allocs until the context goes)
int ensure_red_rows(raocp_ctx* c, int rows) {
    if (rows <= c->red_rows) return RAOCP_OK;
    c->red_rows = rows;
    if (int rc = c->alloc(&c->redpart, (size_t)c->red_rows * 6)) return rc;
    if (hipMemset(c->redpart, 0, (size_t)c->red_rows * 6 * sizeof(double)) != hipSuccess) return fail(RAOCP_ERR_HIP, "memset");
    return RAOCP_OK;
}

// the device's CU count (256 when the query fails)
int device_cus(int device) {
    int n_cus = 0;
    if (hipDeviceGetAttribute(&n_cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n_cus <= 0) n_cus = 256;
    return n_cus;
}

// ---- node-block CP tables (raocp_cp.hip) for given owned parent / leaf id ranges ----
struct CpFam { int cb, ce, y0, y1, e7a, e7b; };
CpFam cp_fam(const raocp_ctx* c, int i0, int i1) {
    CpFam f;
    f.cb = c->h_chs[i0];
    f.ce = c->h_chs[i1 - 1] + c->h_nch[i1 - 1];
    f.y0 = c->h_yrel[i0];
    f.y1 = c->h_yrel[i1 - 1] + 2 * c->h_nch[i1 - 1] + 1;
    f.e7a = c->h_pos7[i0];
    f.e7b = c->h_pos7[i1];
    return f;
}

// LDS doubles of one block (k_cpd, k_cpp), mirroring the Stg regions of raocp_cp.hip
std::pair<long, long> cp_block_need(const raocp_ctx* c, bool family, int a0, int a1) {
    const long nx = c->nx, nu = c->nu;
    auto dbl = [](long cnt) { return (cnt + 1) / 2 * 2 + 2; };
    auto recs = [](long cnt) { return 2 * cnt + 2; };
    auto ints = [](long cnt) { return (cnt * 4 + 22) / 8 / 2 * 2 + 4; };
    const long nQ = (long)c->n_sq * nx * nx, nR = (long)c->n_sr * nu * nu, nP = (long)c->n_sp * nx * nx;
    const long nBx = (long)c->nbn * (nx + nu), nBlx = (long)c->nbl * nx;
    if (family) {
        const long P = a1 - a0;
        const CpFam f = cp_fam(c, a0, a1);
        const long C = f.ce - f.cb, Y = f.y1 - f.y0, E7n = f.e7b - f.e7a;
        const long nd = 2 * dbl(P * nx) + 2 * dbl(P * nu) + 2 * dbl(Y) + 2 * dbl(P) + 2 * dbl(C) + dbl(C) + dbl(Y) +
                        dbl(P) + dbl(E7n) + dbl(C * nx) + dbl(C * nu) + 2 * dbl(C) + recs(P) + recs(C) + ints(P) +
                        dbl(nQ) + dbl(nR) + 2 * dbl(nBx);
        const long npp = 3 * (dbl(Y) + dbl(P) + dbl(C * nx) + dbl(C * nu) + 2 * dbl(C) + dbl(E7n) + 3 * dbl(C)) +
                         2 * dbl(P * nx) + 2 * dbl(P * nu) + 2 * dbl(Y) + 2 * dbl(C) + 2 * dbl(C) + dbl(C) + dbl(P) +
                         recs(P) + recs(C) + dbl(nQ) + dbl(nR);
        return {nd, npp};
    }
    const long Lc = a1 - a0;
    const long E14n = c->h_pos14[a1 - c->m] - c->h_pos14[a0 - c->m];
    const long nd = 2 * dbl(Lc * nx) + 2 * dbl(Lc) + dbl(Lc * nx) + 2 * dbl(Lc) + dbl(E14n) + recs(Lc) + dbl(nP) +
                    2 * dbl(nBlx);
    const long npp = 3 * (dbl(Lc * nx) + dbl(E14n)) + 2 * dbl(Lc * nx) + recs(Lc) + dbl(nP);
    return {nd, npp};
}

long cp_need(const raocp_ctx* c, const std::vector<std::pair<int, int>>& pr_, const std::vector<std::pair<int, int>>& lr_,
             int FB, int LB) {
    long w = 0;
    for (const auto& r : pr_)
        for (int i0 = r.first; i0 < r.second; i0 += FB) {
            const auto nd = cp_block_need(c, true, i0, std::min(r.second, i0 + FB));
            w = std::max(w, std::max(nd.first, nd.second));
        }
    for (const auto& r : lr_)
        for (int l0 = r.first; l0 < r.second; l0 += LB) {
            const auto nd = cp_block_need(c, false, l0, std::min(r.second, l0 + LB));
            w = std::max(w, std::max(nd.first, nd.second));
        }
    return w;
}

// ---- MFMA CP blocks (raocp_cp2.hip): LDS bytes of one block, mirroring StgB (worst-case
// misalignment of each region: 15 B)
long cp2_region(long nbytes) { return nbytes > 0 ? 16 * ((nbytes + 30) >> 4) + 16 : 16; }
std::pair<long, long> cp2_block_need(const raocp_ctx* c, bool family, int a0, int a1, bool regular) {
    const long nx = c->nx, nu = c->nu, w = c->wsz;
    auto R = [&](long cnt) { return cp2_region(cnt * w); };
    auto Rr = [&](long cnt) { return cp2_region(cnt * 16); };
    auto Ri = [&](long cnt) { return cp2_region(cnt * 4); };
    const long nBx = (long)c->nbn * (nx + nu), nBlx = (long)c->nbl * nx;
    if (family) {
        const long P = a1 - a0;
        const CpFam f = cp_fam(c, a0, a1);
        const long C = f.ce - f.cb, Y = f.y1 - f.y0, E7n = f.e7b - f.e7a;
        const long nd = 2 * R(P * nx) + 2 * R(P * nu) + 2 * R(Y) + 2 * R(P) + 3 * R(C) + R(Y) + R(P) + R(E7n) +
                        R(C * nx) + R(C * nu) + 2 * R(C) + Rr(P) + Rr(C) + Ri(P) + 2 * R(nBx);
        long npp = 3 * (R(Y) + R(P) + R(C * nx) + R(C * nu) + 2 * R(C) + R(E7n) + 3 * R(C)) + 2 * R(P * nx) +
                   2 * R(P * nu) + 2 * R(Y) + 5 * R(C) + R(P) + Rr(P) + Rr(C);
        if (!regular) npp += 3 * C * (nx + nu) * w;
        return {nd, npp};
    }
    const long Lc = a1 - a0;
    const long E14n = c->h_pos14[a1 - c->m] - c->h_pos14[a0 - c->m];
    const long nd = 2 * R(Lc * nx) + 2 * R(Lc) + R(Lc * nx) + 2 * R(Lc) + R(E14n) + Rr(Lc) + 2 * R(nBlx);
    const long npp = 3 * (R(Lc * nx) + R(E14n)) + 2 * R(Lc * nx) + Rr(Lc);
    return {nd, npp};
}

// largest LDS bytes of a MFMA CP block over a range of parents (families of FB) or leaves (LB)
long cp2_need(const raocp_ctx* c, int a, int b, int per, bool family);

// the uniform table index of nodes [a, b) (-1 when they differ or the range is empty)
int uniform_idx(const std::vector<int>& idx, int a, int b) {
    if (b <= a) return -1;
    for (int q = a + 1; q < b; ++q)
        if (idx[q] != idx[a]) return -1;
    return idx[a];
}

bool cp2_regular(const raocp_ctx* c, int i0, int i1) {
    const CpFam f = cp_fam(c, i0, i1);
    int creg = c->h_nch[i0] <= 4 ? c->h_nch[i0] : 0;
    for (int q = i0; q < i1 && creg; ++q)
        if (c->h_nch[q] != creg || c->h_chs[q] != f.cb + (q - i0) * creg) creg = 0;
    return creg > 0 && uniform_idx(c->h_isq, f.cb, f.ce) >= 0 && uniform_idx(c->h_isr, f.cb, f.ce) >= 0;
}
long cp2_need(const raocp_ctx* c, int a, int b, int per, bool family) {
    long w = 0;
    for (int x0 = a; x0 < b; x0 += per) {
        const int x1 = std::min(b, x0 + per);
        const auto nd = cp2_block_need(c, family, x0, x1, family ? cp2_regular(c, x0, x1) : true);
        w = std::max(w, std::max(nd.first, nd.second));
    }
    return w;
}

// (re)build the CP block table for the owned parent ranges and leaf ranges
int build_cp_blocks(raocp_ctx* c, const std::vector<std::pair<int, int>>& pranges,
                    const std::vector<std::pair<int, int>>& lranges) {
    std::vector<raocp::Rec> fam, leaf;
    long need_d = 0, need_p = 0;
    for (const auto& r : pranges)
        for (int i0 = r.first; i0 < r.second; i0 += c->cp_FB) {
            const int i1 = std::min(r.second, i0 + c->cp_FB);
            const CpFam f = cp_fam(c, i0, i1);
            fam.push_back(raocp::Rec{f.cb, f.ce, f.y0, f.y1});
            fam.push_back(raocp::Rec{f.e7a, f.e7b, i0, i1});
            const auto nd = cp_block_need(c, true, i0, i1);
            need_d = std::max(need_d, nd.first);
            need_p = std::max(need_p, nd.second);
        }
    for (const auto& r : lranges)
        for (int l0 = r.first; l0 < r.second; l0 += c->cp_LB) {
            const int l1 = std::min(r.second, l0 + c->cp_LB);
            leaf.push_back(raocp::Rec{c->h_pos14[l0 - c->m], c->h_pos14[l1 - c->m], l0, l1});
            const auto nd = cp_block_need(c, false, l0, l1);
            need_d = std::max(need_d, nd.first);
            need_p = std::max(need_p, nd.second);
        }
    if (std::max(need_d, need_p) * 8 > 150 * 1024)
        return fail(RAOCP_ERR_ARG, "CP node block does not fit LDS (nx, nu or branching too large)");
    std::vector<raocp::Rec> tab = fam;
    tab.insert(tab.end(), leaf.begin(), leaf.end());
    if (tab.empty()) tab.push_back(raocp::Rec{0, 0, 0, 0});
    const raocp::Rec* dtab = nullptr;
    int rc = c->upload_vec(&dtab, tab);
    if (rc) return rc;
    c->dev.cpd_tab = dtab;
    c->cp_nbF = (int)fam.size() / 2;
    c->cp_nbL = (int)leaf.size();
    c->lds_cpd = (size_t)need_d * 8;
    c->lds_cpp = (size_t)need_p * 8;
    c->cp_rows = c->cp_nbF + c->cp_nbL;
    // MFMA CP blocks (raocp_cp2.hip) over the same ranges
    {
        std::vector<raocp::Rec> fam2, leaf2;
        long nd2 = 0, np2 = 0;
        for (const auto& r : pranges)
            for (int i0 = r.first; i0 < r.second; i0 += c->cp2_FB) {
                const int i1 = std::min(r.second, i0 + c->cp2_FB);
                const CpFam f = cp_fam(c, i0, i1);
                // regular: every parent has the same child count creg <= 4, children in parent order
                int creg = c->h_nch[i0] <= 4 ? c->h_nch[i0] : 0;
                for (int q = i0; q < i1 && creg; ++q)
                    if (c->h_nch[q] != creg || c->h_chs[q] != f.cb + (q - i0) * creg) creg = 0;
                fam2.push_back(raocp::Rec{f.cb, f.ce, f.y0, f.y1});
                fam2.push_back(raocp::Rec{f.e7a, f.e7b, i0, i1});
                const int tq = uniform_idx(c->h_isq, f.cb, f.ce), tr = uniform_idx(c->h_isr, f.cb, f.ce);
                fam2.push_back(raocp::Rec{tq, tr, creg, 0});
                const auto nd = cp2_block_need(c, true, i0, i1, creg > 0 && tq >= 0 && tr >= 0);
                nd2 = std::max(nd2, nd.first);
                np2 = std::max(np2, nd.second);
            }
        for (const auto& r : lranges)
            for (int l0 = r.first; l0 < r.second; l0 += c->cp2_LB) {
                const int l1 = std::min(r.second, l0 + c->cp2_LB);
                leaf2.push_back(raocp::Rec{c->h_pos14[l0 - c->m], c->h_pos14[l1 - c->m], l0, l1});
                leaf2.push_back(raocp::Rec{uniform_idx(c->h_isp, l0, l1), 0, 0, 0});
                const auto nd = cp2_block_need(c, false, l0, l1, true);
                nd2 = std::max(nd2, nd.first);
                np2 = std::max(np2, nd.second);
            }
        if (std::max(nd2, np2) > 150 * 1024)
            return fail(RAOCP_ERR_ARG, "MFMA CP block does not fit LDS (nx, nu or branching too large)");
        std::vector<raocp::Rec> tab2 = fam2;
        tab2.insert(tab2.end(), leaf2.begin(), leaf2.end());
        if (tab2.empty()) tab2.push_back(raocp::Rec{0, 0, 0, 0});
        const raocp::Rec* dtab2 = nullptr;
        if ((rc = c->upload_vec(&dtab2, tab2))) return rc;
        c->dev.cp2_tab = dtab2;
        c->cp2_nbF = (int)fam2.size() / raocp::kCpFamRecs;
        c->cp2_nbL = (int)leaf2.size() / raocp::kCpLeafRecs;
        // the MFMA kernels need every block's nodes on one weight table (per-mode tables the
        // packer could not merge): otherwise the scalar kernels (raocp_cp.hip) run
        for (int b = 0; b < c->cp2_nbF; ++b)
            if (fam2[raocp::kCpFamRecs * b].y > fam2[raocp::kCpFamRecs * b].x &&
                (fam2[raocp::kCpFamRecs * b + 2].x < 0 || fam2[raocp::kCpFamRecs * b + 2].y < 0))
                c->cp_v1 = c->ell2_mixed = true;
        for (int b = 0; b < c->cp2_nbL; ++b)
            if (leaf2[raocp::kCpLeafRecs * b + 1].x < 0) c->cp_v1 = c->ell2_mixed = true;
        c->lds_cpd2 = (size_t)nd2;
        c->lds_cpp2 = (size_t)np2;
        c->cp_rows = c->cp_v1 ? c->cp_nbF + c->cp_nbL : c->cp2_nbF + c->cp2_nbL;
    }
    return RAOCP_OK;
}

// ---- the regular-tree sweep (raocp_dynr.hip) -----------------------------------------------
// Tables in the kernel's LDS order, per nonleaf stage t (its class and the pairs of its child
// slots, c->reg_st[t]), element-pair-major [p][lane][2] so lane s reads its row pair p as one
// 16-B word:
//   backward lane s = r KS + k (row r < nx + nu, slot k; LB = (nx + nu) KS lanes): WT = [-Rinv B' ; A' - G B'] row r of
//            slot k's pair (zero for k >= C), then entries [k UP, (k + 1) UP) of RG = [Rinv ; G]
//            row r of the class;
//   forward  lane s = k nx + r (slot k, row r < nx; LF = C nx + nu lanes): [Abar_k | B_k] row r; lane C nx + r
//            (r < nu): [K row r | unit vector e_r] (u_r = K x + d_r as one dot product).
// The tier plan minimises a cost model of the critical path (us, fitted to measured cut lists:
// per level of each sweep a fixed part and a part per node, per tier boundary its two
// hand-offs) over cut lists of at most kDrMaxTiers tiers whose grid (one workgroup per subtree
// of every tier, plus the stopping test) is resident at once (occupancy x CU count): no wait
// then depends on the dispatch order. RAOCP_DR_CUTS="s1:s2:.." forces the cuts.
int dr_setup(raocp_ctx* c, const DynTables& dt, int n_cus) {
    const std::vector<double>&WT = dt.WT, &RG = dt.RG, &KM = dt.KM, &F = dt.F;
    const int SKP = dt.SKP, SNU = dt.SNU, SKF = dt.SKF;
    const int nx = c->nx, nu = c->nu, C = c->reg_C, N = c->N, R = nx + nu;
    const int KS = raocp::dr_ks(C), UP = raocp::dr_up(nu, C), LB = raocp::dr_lb(nx, nu, C),
              LF = raocp::dr_lf(nx, nu, C);
    const int nb = raocp::dr_tb_n(nx, nu, C), nf = raocp::dr_tf_n(nx, nu, C);
    auto npow = [&](int e) {
        long v = 1;
        for (int i = 0; i < e; ++i) v *= C;
        return v;
    };
    if (N >= raocp::kDrMaxStages) return RAOCP_OK;  // the sweep stays off
    int block = 512;
    // cost (us) of a cut list s = {0, s1, .., N}; 1e300 where it does not fit
    auto eval = [&](const std::vector<int>& s) -> double {
        const int T = (int)s.size() - 1;
        if (T < 1 || T > raocp::kDrMaxTiers) return 1e300;
        long wgs = 1;  // the stopping test
        size_t lds = 0;
        int lmax = 0;
        for (int k = 0; k < T; ++k) {
            const int L = s[k + 1] - s[k];
            if (L < 1 || L > raocp::kDrMaxL) return 1e300;
            lmax = std::max(lmax, L);
            wgs += npow(s[k]);
            lds = std::max(lds, raocp::dr_lds(nx, nu, C, L));
            if (k + 1 < T && npow(L) * 2 * nx > (long)raocp::kDrMaxGran * block) return 1e300;
        }
        if (lds > 160 * 1024 - 512) return 1e300;
        const int occ = raocp::dr_occupancy(nx, nu, C, lmax, lds);
        if (occ < 1 || wgs > (long)occ * n_cus) return 1e300;
        // fitted to the config-2 cut lists measured on MI355X (profiles/r04_*/dr_cuts.log): a
        // level 0.6 us plus 0.045 us per node beyond the first, each way; a tier boundary
        // 2.5 us (its two hand-offs)
        double cost = 2.5 * (T - 1);
        for (int k = 0; k < T; ++k)
            for (int l = 0; l < s[k + 1] - s[k]; ++l) cost += 2 * (0.6 + 0.045 * (double)(npow(l) - 1));
        return cost;
    };
    std::vector<int> cuts;
    if (const char* e = getenv("RAOCP_DR_CUTS")) {
        cuts.push_back(0);
        for (const char* p = e; *p;) {
            char* q = nullptr;
            const long v = strtol(p, &q, 10);
            if (q == p) break;
            if (v > 0 && v < N) cuts.push_back((int)v);
            p = *q ? q + 1 : q;
        }
        cuts.push_back(N);
        if (!std::is_sorted(cuts.begin(), cuts.end()) || eval(cuts) >= 1e299)
            return fail(RAOCP_ERR_ARG, std::string("RAOCP_DR_CUTS=") + e + ": not a valid tier plan for this tree");
    } else {
        double best = 1e300;
        std::vector<int> s{0};
        // every increasing cut list of at most kDrMaxTiers tiers
        auto rec = [&](auto&& self, int from) -> void {
            s.push_back(N);
            const double v = eval(s);
            if (v < best) {
                best = v;
                cuts = s;
            }
            s.pop_back();
            if ((int)s.size() >= raocp::kDrMaxTiers) return;
            for (int a = from; a < N; ++a) {
                s.push_back(a);
                self(self, a + 1);
                s.pop_back();
            }
        };
        rec(rec, 1);
        if (best >= 1e299) return RAOCP_OK;  // no plan: the sweep stays off
    }
    std::vector<double> bimg((size_t)N * nb, 0.0), fimg((size_t)N * nf, 0.0);
    for (int t = 0; t < N; ++t) {
        const raocp::Dy3Stage& st = c->reg_st[t];
        double* b = &bimg[(size_t)t * nb];
        auto bset = [&](int e, int lane, double v) { b[((size_t)(e / 2) * LB + lane) * 2 + (e & 1)] = v; };
        for (int r = 0; r < R; ++r)
            for (int k = 0; k < KS; ++k) {
                const int lane = r * KS + k;
                if (k < C)
                    for (int e = 0; e < nx; ++e) bset(e, lane, WT[((size_t)st.pair[k] * R + r) * SKP + e]);
                for (int e = 0; e < UP && k * UP + e < nu; ++e)
                    bset(nx + e, lane, RG[((size_t)st.cls * R + r) * SNU + k * UP + e]);
            }
        double* f = &fimg[(size_t)t * nf];
        auto fset = [&](int e, int lane, double v) { f[((size_t)(e / 2) * LF + lane) * 2 + (e & 1)] = v; };
        for (int k = 0; k < C; ++k)
            for (int r = 0; r < nx; ++r)
                for (int e = 0; e < nx + nu; ++e) fset(e, k * nx + r, F[((size_t)st.pair[k] * nx + r) * SKF + e]);
        for (int r = 0; r < nu; ++r) {
            for (int e = 0; e < nx; ++e) fset(e, C * nx + r, KM[((size_t)st.cls * nu + r) * SKP + e]);
            fset(nx + r, C * nx + r, 1.0);
        }
    }
    raocp::DrPlan& p = c->drp;
    memset(&p, 0, sizeof(p));
    const int T = (int)cuts.size() - 1;
    p.T = T;
    p.C = C;
    p.N = N;
    int w = 0, b0 = 0;
    for (int k = T - 1; k >= 0; --k) {  // the deepest tier first, the top last
        p.t[k].b0 = b0;
        b0 += (int)npow(cuts[k]);
    }
    c->dr_lds = 0;
    for (int k = 0; k < T; ++k) {
        raocp::DrTier& tt = p.t[k];
        tt.s0 = cuts[k];
        tt.L = cuts[k + 1] - cuts[k];
        tt.nsub = (int)npow(cuts[k]);
        tt.w0 = w;
        w += tt.nsub;
        c->dr_lds = std::max(c->dr_lds, raocp::dr_lds(nx, nu, C, tt.L));
    }
    p.nblk = b0;
    for (int t = 0; t <= N; ++t) p.sbase[t] = (int)((npow(t) - 1) / (C - 1));
    p.X0 = c->dev.X0;
    p.U0 = c->dev.U0;
    c->dr_block = block;
    // error-path test (tests/test_gpu_dynr.py): RAOCP_DR_FAULT=1 makes the deepest tier's first
    // subtree skip its publish, so its parent's wait times out and the call fails; the
    // timing-only bits (no DMA / arithmetic / write-out) exist in diagnostic builds only
    // (the timing bits pass where the sweep's unit is a diagnostic build: VAR_UNIT=dynr variants)
    p.fault = env_int("RAOCP_DR_FAULT", 0) & ((raocp::kDiag || raocp::dr_diag_build()) ? ~0 : 1);
    // composed maps (raocp_drxfer.h), from the arrays the stage tables above come from: a tier
    // between the top and the deepest, of binary subtrees with 4 levels at 20 / 8, publishes its
    // root's q row from one composed product before its backward levels. One map per such tier
    // (one class per stage and one pair per slot: every subtree of a tier shares it), uploaded
    // once. RAOCP_DR_XFER=0 keeps every row level by level.
    const bool xfer = env_flag("RAOCP_DR_XFER", true);
    std::vector<double> xbq;
    int lmax = 0;
    for (int k = 0; k < T; ++k) lmax = std::max(lmax, p.t[k].L);
    // (plans of at most 4 levels per tier: the kernel compiled for them holds the composed step)
    if (xfer && C == 2 && nx == raocp::kXbNx && nu == raocp::kXbNu && T > 2 && lmax <= 4) {
        xbq.assign((size_t)(T - 2) * raocp::kDrXbN, 0.0);
        for (int k = 1; k + 1 < T; ++k) {
            if (p.t[k].L != raocp::kXbL) continue;
            raocp::XbStages xs;
            xs.sphi = SKP;
            xs.srg = SNU;
            for (int l = 0; l < raocp::kXbL; ++l) {
                const raocp::Dy3Stage& st = c->reg_st[p.t[k].s0 + l];
                for (int q = 0; q < 2; ++q) xs.phi[l][q] = &WT[((size_t)st.pair[q] * R + nu) * SKP];
                xs.rgq[l] = &RG[((size_t)st.cls * R + nu) * SNU];
            }
            raocp::xb_pack(raocp::xb_compose(xs), &xbq[(size_t)(k - 1) * raocp::kDrXbN]);
            p.t[k].xf |= raocp::kDrXfMidBack;
        }
    }
    // the forward maps: every tier below the top (the deepest included) of binary subtrees with 4
    // levels sweeps forward from a zero root row inside its wait for that row and adds the
    // composed map times the row when it lands. RAOCP_DR_FWD=0 switches off these alone.
    const bool fwd = xfer && env_flag("RAOCP_DR_FWD", true);
    std::vector<double> xfw;
    if (fwd && C == 2 && nx == raocp::kXbNx && nu == raocp::kXbNu && T > 1 && lmax <= 4 && block == raocp::kXfL1) {
        xfw.assign((size_t)(T - 1) * raocp::kDrXfN, 0.0);
        for (int k = 1; k < T; ++k) {
            if (p.t[k].L != raocp::kXbL) continue;
            raocp::XfStages xs;
            xs.sab = SKF;
            xs.skm = SKP;
            for (int l = 0; l < raocp::kXbL; ++l) {
                const raocp::Dy3Stage& st = c->reg_st[p.t[k].s0 + l];
                for (int q = 0; q < 2; ++q) xs.ab[l][q] = &F[(size_t)st.pair[q] * nx * SKF];
                xs.km[l] = &KM[(size_t)st.cls * nu * SKP];
            }
            raocp::xf_pack(raocp::xf_compose(xs), &xfw[(size_t)(k - 1) * raocp::kDrXfN]);
            p.t[k].xf |= raocp::kDrXfFwd;
        }
    }
    int rc;
    const double *bi = nullptr, *fi = nullptr, *xq = nullptr, *xw = nullptr;
    unsigned long long *gq = nullptr, *gx = nullptr;
    unsigned* sy = nullptr;
    c->dr_gran = (size_t)w * 2 * nx;
    if ((rc = c->upload_vec(&bi, bimg)) || (rc = c->upload_vec(&fi, fimg)) || (rc = c->alloc(&gq, c->dr_gran)) ||
        (rc = c->alloc(&gx, c->dr_gran)) || (rc = c->alloc(&sy, 2)))
        return rc;
    HIPCHK(hipMemset(sy, 0, 2 * sizeof(unsigned)));
    HIPCHK(hipMemset(gq, 0, c->dr_gran * sizeof(unsigned long long)));
    HIPCHK(hipMemset(gx, 0, c->dr_gran * sizeof(unsigned long long)));
    if (!xbq.empty() && (rc = c->upload_vec(&xq, xbq))) return rc;
    p.bimg = bi;
    p.fimg = fi;
    if (!xfw.empty() && (rc = c->upload_vec(&xw, xfw))) return rc;
    p.xbq = xq;
    p.xfw = xw;
    p.gq = gq;
    p.gx = gx;
    p.sync = sy;
    p.timeout = fuse_timeout_ticks();
    c->dr = true;
    return RAOCP_OK;
}

// k_drc (raocp_dynr.hip): where k_dr and k_cp6 both run and every tier of the plan has 4 levels
// (binary trees, 20 / 8, fp64, every node boxed or none), the fused launch replaces the pair;
// RAOCP_DRC=0 keeps them. Its weight image is k_cp3's [sqrtQ | sqrtR | sqrtPf] followed by the
// one box table of each kind [lo_nl | hi_nl | lo_l | hi_l] (zeros when unboxed); its residual rows
// are two sets of one row per sweep wave (8 per workgroup, drc_part).
int drc_setup(raocp_ctx* c, int n_cus) {
    c->drc = false;
    if (!c->dr || !c->cp6 || c->f32 || c->sh_S > 0 || !raocp::drc_supported(c->nx, c->nu, c->reg_C)) return RAOCP_OK;
    if (!env_flag("RAOCP_DRC", true)) return RAOCP_OK;
    const raocp::DrPlan& p = c->drp;
    for (int k = 0; k < p.T; ++k)
        if (p.t[k].L != 4) return RAOCP_OK;
    const int bx = c->box_mode;
    if (bx != 5 && bx != 10) return RAOCP_OK;
    const size_t lds = raocp::drc_lds(c->nx, c->nu, 2);
    const int occ = raocp::drc_occupancy(lds);
    if (occ < 1 || (long)p.nblk + 1 > (long)occ * n_cus) return RAOCP_OK;  // the grid must be resident
    const int nx = c->nx, nu = c->nu, R = nx + nu;
    const size_t nimg = raocp::kDrcWa + raocp::kDrcWb;
    double* img = nullptr;
    int rc;
    if ((rc = c->alloc(&img, nimg))) return rc;
    HIPCHK(hipMemset(img, 0, nimg * sizeof(double)));
    HIPCHK(hipMemcpy(img, c->cp3img, (size_t)(raocp::kDrcWa + 640) * sizeof(double), hipMemcpyDeviceToDevice));
    if ((bx & 3) == 1) {
        double* bx0 = img + raocp::kDrcWa + 640;
        HIPCHK(hipMemcpy(bx0, c->dev.blo_nl, R * sizeof(double), hipMemcpyDeviceToDevice));
        HIPCHK(hipMemcpy(bx0 + R, c->dev.bhi_nl, R * sizeof(double), hipMemcpyDeviceToDevice));
        HIPCHK(hipMemcpy(bx0 + 2 * R, c->dev.blo_l, nx * sizeof(double), hipMemcpyDeviceToDevice));
        HIPCHK(hipMemcpy(bx0 + 2 * R + nx, c->dev.bhi_l, nx * sizeof(double), hipMemcpyDeviceToDevice));
    }
    const int rows = 8 * p.nblk;
    if ((rc = ensure_red_rows(c, 2 * rows))) return rc;
    c->cp_rows = rows;
    raocp::DrcArg& a = c->drca;
    const raocp::Dev& D = c->dev;
    a = raocp::DrcArg{};
    a.m = c->m;
    a.Y0 = D.Y0;
    a.T0 = D.T0;
    a.S0 = D.S0;
    a.E1 = D.E1; a.E2 = D.E2; a.E3 = D.E3; a.E4 = D.E4; a.E5 = D.E5; a.E6 = D.E6; a.E7 = D.E7;
    a.E11 = D.E11; a.E12 = D.E12; a.E13 = D.E13; a.E14 = D.E14;
    a.cond = D.cond;
    a.alpha_r = D.alpha_r;
    a.blo_nl = D.blo_nl; a.bhi_nl = D.bhi_nl; a.blo_l = D.blo_l; a.bhi_l = D.bhi_l;
    a.img = img;
    a.ctl = c->ctl;
    a.box = (bx & 3) == 1 ? 1 : 2;
    // the unboxed k_drc holds no forward-map step (it does not fit its 128 VGPRs without a
    // spill): the context's plan, shared with k_dr, keeps the level path there
    if (a.box == 2)
        for (int k = 0; k < c->drp.T; ++k) c->drp.t[k].xf &= ~raocp::kDrXfFwd;
    // the launch's arguments in device memory, one copy per iteration parity (part / nanbit)
    {
        raocp::DrcArg two[2] = {a, a};
        for (int q = 0; q < 2; ++q) {
            two[q].part = drc_part(c, q);
            two[q].nanbit = drc_nanbit(q);
        }
        double* d = nullptr;
        const size_t words = (2 * sizeof(raocp::DrcArg) + 7) / 8;
        if ((rc = c->alloc(&d, words))) return rc;
        HIPCHK(hipMemcpy(d, two, sizeof(two), hipMemcpyHostToDevice));
        c->d_drca = (raocp::DrcArg*)d;
    }
    c->drc_lds = lds;
    c->drc = true;
    return RAOCP_OK;
}

// ---- the stages of raocp_ctx_create, in the order it runs them -----------------------------

// ---- validate the layout invariants the kernels rely on (no HIP call)
int validate_tree(const raocp_tree_desc* t, int* N_out, int* cmax_out) {
    const int n = t->n, m = t->m, nx = t->nx, nu = t->nu;
    if (n < 2 || m < 1 || m >= n || nx < 1 || nu < 1) return fail(RAOCP_ERR_ARG, "bad tree sizes");
    // the MFMA CP kernels are instantiated for up to 4 row tiles of nx and 2 of nu (dispatch_rt)
    if (nx > 64 || nu > 32) return fail(RAOCP_ERR_ARG, "the CP kernels support nx <= 64 and nu <= 32");
    if (t->anc[0] != -1 || t->stage[0] != 0) return fail(RAOCP_ERR_TREE, "node 0 must be the root");
    for (int i = 1; i < n; ++i) {
        if (t->stage[i] < t->stage[i - 1]) return fail(RAOCP_ERR_TREE, "stage must be non-decreasing in node id");
        if (t->anc[i] < 0 || t->anc[i] >= i) return fail(RAOCP_ERR_TREE, "ancestor must precede its child");
    }
    const int N = t->stage[n - 1];
    int expect = 1, cmax = 0;
    for (int i = 0; i < m; ++i) {
        if (t->stage[i] >= N) return fail(RAOCP_ERR_TREE, "nonleaf nodes must be ids 0..m-1");
        if (t->nch[i] < 1 || t->ch_start[i] != expect)
            return fail(RAOCP_ERR_TREE, "children must be contiguous id ranges in parent order");
        for (int k = 0; k < t->nch[i]; ++k)
            if (t->anc[expect + k] != i || t->stage[expect + k] != t->stage[i] + 1)
                return fail(RAOCP_ERR_TREE, "child range inconsistent with ancestors/stages");
        expect += t->nch[i];
        cmax = std::max(cmax, (int)t->nch[i]);
    }
    if (expect != n) return fail(RAOCP_ERR_TREE, "children ranges do not cover nodes 1..n-1");
    for (int i = m; i < n; ++i)
        if (t->stage[i] != N) return fail(RAOCP_ERR_TREE, "leaves must all be at the last stage");
    // group sizes of every kernel must fit one workgroup
    int rc;
    if ((rc = check_group(nx + nu + 2, "child block")) || (rc = check_group(2 * cmax + 2 + nx + nu, "nonleaf block")) ||
        (rc = check_group(2 * nx + 2, "leaf block")) || (rc = check_group(nx + nu + 2 * cmax + 2 + cmax, "L^T nonleaf")) ||
        (rc = check_group(nx + nu + cmax + 1, "CP primal nonleaf")))
        return rc;
    *N_out = N;
    *cmax_out = cmax;
    return RAOCP_OK;
}

// ---- flat layout (cache.py:126-170)
int layout_vectors(raocp_ctx* c, const raocp_tree_desc* t, const raocp_problem_desc* pr, Layout& lay) {
    const int n = c->n, m = c->m, nx = c->nx, nu = c->nu, cmax = c->cmax, N = c->N;
    c->stage_ptr.assign(N + 2, n);
    for (int i = n - 1; i >= 0; --i) c->stage_ptr[t->stage[i]] = i;
    c->stage_ptr[N + 1] = n;

    Dev& D = c->dev;
    D.n = n; D.m = m; D.nx = nx; D.nu = nu; D.cmax = cmax;
    std::vector<int>&yrel = lay.yrel, &e7off = lay.e7off, &e14off = lay.e14off, &rank = lay.rank, &ph = lay.ph;
    yrel.assign(m, 0);
    e7off.assign(m, -1);
    e14off.assign(n - m, -1);
    rank.assign(n, 0);
    int ysum = 0;
    for (int i = 0; i < m; ++i) {
        yrel[i] = ysum;
        ysum += 2 * t->nch[i] + 1;
        for (int k = 0; k < t->nch[i]; ++k) rank[t->ch_start[i] + k] = k;
    }
    int64_t off = 0;
    D.X0 = (int)off; off += (int64_t)n * nx;
    D.U0 = (int)off; off += (int64_t)m * nu;
    D.Y0 = (int)off; off += ysum;
    D.T0 = (int)off; off += n;
    D.S0 = (int)off; off += n;
    c->P = off; D.P = (int)off;
    off = 0;
    D.E1 = (int)off; off += ysum + (n - m);
    D.E2 = (int)off; off += n;
    D.E3 = (int)off; off += 1 + (int64_t)(n - 1) * nx;
    D.E4 = (int)off; off += 1 + (int64_t)(n - 1) * nu;
    D.E5 = (int)off; off += n;
    D.E6 = (int)off; off += n;
    D.E7 = (int)off;
    for (int i = 0; i < n; ++i) {
        if (i < m && pr->i_box_nl[i] >= 0) { e7off[i] = (int)off; off += nx + nu; }
        else off += 1;
    }
    D.E11 = (int)off; off += m + (int64_t)(n - m) * nx;
    D.E12 = (int)off; off += n;
    D.E13 = (int)off; off += n;
    D.E14 = (int)off;
    for (int i = 0; i < n; ++i) {
        if (i >= m && pr->i_box_l[i] >= 0) { e14off[i - m] = (int)off; off += nx; }
        else off += 1;
    }
    c->D = off; D.D = (int)off;
    // dual placeholders: (1,1) blocks no projection touches; prox_g* maps them to exactly 0
    for (int l = m; l < n; ++l) ph.push_back(D.E1 + ysum + (l - m));
    for (int l = m; l < n; ++l) ph.push_back(D.E2 + l);
    ph.push_back(D.E3); ph.push_back(D.E4); ph.push_back(D.E5); ph.push_back(D.E6);
    {
        int o = D.E7;
        for (int i = 0; i < n; ++i) {
            if (i < m && e7off[i] >= 0) o += nx + nu;
            else ph.push_back(o++);
        }
        o = D.E14;
        for (int i = 0; i < n; ++i) {
            if (i >= m && e14off[i - m] >= 0) o += nx;
            else ph.push_back(o++);
        }
    }
    for (int i = 0; i < m; ++i) { ph.push_back(D.E11 + i); ph.push_back(D.E12 + i); ph.push_back(D.E13 + i); }
    if (c->P >= (int64_t)1 << 31 || c->D >= (int64_t)1 << 31)
        return fail(RAOCP_ERR_ARG, "flat vectors exceed 2^31 entries (int32 offsets)");
    return RAOCP_OK;
}

// ---- tables
int upload_cost_tables(raocp_ctx* c, const raocp_tree_desc* t, const raocp_problem_desc* pr, const Layout& lay) {
    const int n = c->n, m = c->m, nx = c->nx, nu = c->nu;
    Dev& D = c->dev;
    int rc;
    const std::vector<int>&yrel = lay.yrel, &e7off = lay.e7off, &e14off = lay.e14off, &rank = lay.rank, &ph = lay.ph;
    std::vector<int> ch_start(t->ch_start, t->ch_start + m), nch(t->nch, t->nch + m), anc(t->anc, t->anc + n);
    c->n_ph = (int)ph.size();
    if ((rc = c->upload_vec(&c->ph, ph))) return rc;
    if ((rc = c->upload_vec(&D.anc, anc)) || (rc = c->upload_vec(&D.ch_start, ch_start)) ||
        (rc = c->upload_vec(&D.nch, nch)) || (rc = c->upload_vec(&D.rank, rank)) || (rc = c->upload_vec(&D.yrel, yrel)) ||
        (rc = c->upload_vec(&D.e7off, e7off)) || (rc = c->upload_vec(&D.e14off, e14off)))
        return rc;
    if ((rc = upload_t(c, &D.SQ, to_colmajor(pr->sqrt_q, pr->n_sq, nx, nx))) ||
        (rc = upload_t(c, &D.SR, to_colmajor(pr->sqrt_r, pr->n_sr, nu, nu))) ||
        (rc = upload_t(c, &D.SP, to_colmajor(pr->sqrt_pf, pr->n_sp, nx, nx))) ||
        (rc = c->upload(&D.SQr, pr->sqrt_q, (size_t)pr->n_sq * nx * nx)) ||
        (rc = c->upload(&D.SRr, pr->sqrt_r, (size_t)pr->n_sr * nu * nu)) ||
        (rc = c->upload(&D.SPr, pr->sqrt_pf, (size_t)pr->n_sp * nx * nx)) ||
        (rc = c->upload(&D.iSQ, pr->i_sq, n)) || (rc = c->upload(&D.iSR, pr->i_sr, n)) ||
        (rc = c->upload(&D.iSP, pr->i_sp, n)) || (rc = upload_t(c, &D.alpha_r, copy_table(pr->alpha_r, m))) ||
        ((D.nSQ = pr->n_sq), (D.nSR = pr->n_sr), (D.nSP = pr->n_sp), false) ||
        (rc = upload_t(c, &D.cond, copy_table(pr->cond, n))))
        return rc;
    const int nbn = c->nbn = std::max(1, pr->n_box_nl), nbl = c->nbl = std::max(1, pr->n_box_l);
    std::vector<double> lo_nl(nbn * (nx + nu), 0.0), hi_nl(nbn * (nx + nu), 0.0), lo_l(nbl * nx, 0.0), hi_l(nbl * nx, 0.0);
    if (pr->n_box_nl) {
        std::copy(pr->box_nl_lo, pr->box_nl_lo + lo_nl.size(), lo_nl.begin());
        std::copy(pr->box_nl_hi, pr->box_nl_hi + hi_nl.size(), hi_nl.begin());
    }
    if (pr->n_box_l) {
        std::copy(pr->box_l_lo, pr->box_l_lo + lo_l.size(), lo_l.begin());
        std::copy(pr->box_l_hi, pr->box_l_hi + hi_l.size(), hi_l.begin());
    }
    if ((rc = upload_t(c, &D.blo_nl, lo_nl)) || (rc = upload_t(c, &D.bhi_nl, hi_nl)) ||
        (rc = upload_t(c, &D.blo_l, lo_l)) || (rc = upload_t(c, &D.bhi_l, hi_l)) ||
        (rc = c->upload(&D.iBnl, pr->i_box_nl, m)) || (rc = c->upload(&D.iBl, pr->i_box_l, n)))
        return rc;
    return RAOCP_OK;
}

int build_dyn_tables(raocp_ctx* c, const raocp_tree_desc* t, const raocp_problem_desc* pr, DynTables& dt) {
    const int n = c->n, m = c->m, nx = c->nx, nu = c->nu, N = c->N;
    Dev& D = c->dev;
    int rc;
    // dynamics tables (raocp_dyn.hip header): per child kind W = [B'; A'], per class
    // RG = [R~^-1; G = M R~^-1 - K'] and K, per (kind, parent class) pair F = [A + B K | B]
    const int R = dt.R = nx + nu;
    const int KP = raocp::rup(nx, 2 * raocp::kKS), KF = raocp::rup(nx + nu, 2 * raocp::kKS), NUP = raocp::rup(nu, 2);
    c->KP = KP; c->KF = KF; c->NUP = NUP; c->PS = NUP + raocp::rup(nx, 2);
    const int SKP = dt.SKP = raocp::tstride(KP), SKF = dt.SKF = raocp::tstride(KF), SNU = dt.SNU = raocp::tstride(NUP);  // table row strides
    if (R * raocp::kKS > raocp::kDynBlock)
        return fail(RAOCP_ERR_ARG, "nx + nu > 256 is not supported by the dynamics sweep");
    const int nk = pr->n_k;
    for (int j = 1; j < n; ++j)
        if (pr->i_a[j] < 0 || pr->i_a[j] >= pr->n_a || pr->i_b[j] < 0 || pr->i_b[j] >= pr->n_b)
            return fail(RAOCP_ERR_ARG, "dynamics index out of range");
    for (int i = 0; i < m; ++i)
        if (pr->i_k[i] < 0 || pr->i_k[i] >= nk) return fail(RAOCP_ERR_ARG, "class index out of range");
    // the plant of a closed-loop simulation (raocp_cp_batch_mpc): per child of the root the
    // doubles of A_i | B_i, and of sqrt Q_i | sqrt R_i for the realised stage cost (row-major)
    c->h_mpc_ab.clear();
    c->h_mpc_w.clear();
    for (int q = 0; q < t->nch[0]; ++q) {
        const int i = t->ch_start[0] + q;
        if (pr->i_sq[i] < 0 || pr->i_sq[i] >= pr->n_sq || pr->i_sr[i] < 0 || pr->i_sr[i] >= pr->n_sr) {
            c->h_mpc_ab.clear();
            c->h_mpc_w.clear();
            break;
        }
        const double* a = pr->A + (size_t)pr->i_a[i] * nx * nx;
        const double* b = pr->B + (size_t)pr->i_b[i] * nx * nu;
        const double* sq = pr->sqrt_q + (size_t)pr->i_sq[i] * nx * nx;
        const double* sr = pr->sqrt_r + (size_t)pr->i_sr[i] * nu * nu;
        c->h_mpc_ab.insert(c->h_mpc_ab.end(), a, a + (size_t)nx * nx);
        c->h_mpc_ab.insert(c->h_mpc_ab.end(), b, b + (size_t)nx * nu);
        c->h_mpc_w.insert(c->h_mpc_w.end(), sq, sq + (size_t)nx * nx);
        c->h_mpc_w.insert(c->h_mpc_w.end(), sr, sr + (size_t)nu * nu);
    }
    auto A = [&](int t, int r, int k) { return pr->A[((size_t)t * nx + r) * nx + k]; };
    auto Bm = [&](int t, int r, int k) { return pr->B[((size_t)t * nx + r) * nu + k]; };
    auto K = [&](int c_, int r, int k) { return pr->K[((size_t)c_ * nu + r) * nx + k]; };
    auto Ri = [&](int c_, int r, int k) { return pr->Rinv[((size_t)c_ * nu + r) * nu + k]; };
    auto M = [&](int c_, int r, int k) { return pr->M[((size_t)c_ * nx + r) * nu + k]; };
    // child kinds (A, B index pairs) and (kind, parent class) pairs
    std::vector<int>&kind = dt.kind, &pair = dt.pair;
    std::vector<std::pair<int, int>>&kinds = dt.kinds, &pairs = dt.pairs;
    kind.assign(n, 0);
    pair.assign(n, 0);
    {
        std::vector<std::pair<std::pair<int, int>, int>> seen_k;
        std::vector<std::pair<std::pair<int, int>, int>> seen_p;
        auto find = [](std::vector<std::pair<std::pair<int, int>, int>>& v, std::pair<int, int> key, int next) {
            for (auto& e : v)
                if (e.first == key) return e.second;
            v.push_back({key, next});
            return next;
        };
        for (int j = 1; j < n; ++j) {
            const std::pair<int, int> kk{pr->i_a[j], pr->i_b[j]};
            const int kid = find(seen_k, kk, (int)kinds.size());
            if (kid == (int)kinds.size()) kinds.push_back(kk);
            kind[j] = kid;
            const std::pair<int, int> pk{kid, pr->i_k[t->anc[j]]};
            const int pid = find(seen_p, pk, (int)pairs.size());
            if (pid == (int)pairs.size()) pairs.push_back(pk);
            pair[j] = pid;
        }
    }
    // number pairs by parent class (so the pairs of a stage range are contiguous)
    {
        std::vector<int> order(pairs.size());
        for (size_t q = 0; q < order.size(); ++q) order[q] = (int)q;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return pairs[a].second < pairs[b].second; });
        std::vector<int> newid(pairs.size());
        std::vector<std::pair<int, int>> sorted(pairs.size());
        for (size_t q = 0; q < order.size(); ++q) {
            newid[order[q]] = (int)q;
            sorted[q] = pairs[order[q]];
        }
        pairs = sorted;
        for (int j = 1; j < n; ++j) pair[j] = newid[pair[j]];
    }
    // classes must be numbered by stage: stage t owns classes [cls_ptr[t], cls_ptr[t+1])
    c->cls_ptr.assign(N + 1, nk);
    for (int i = m - 1; i >= 0; --i) c->cls_ptr[t->stage[i]] = std::min(c->cls_ptr[t->stage[i]], pr->i_k[i]);
    for (int st = N - 1; st >= 0; --st) c->cls_ptr[st] = std::min(c->cls_ptr[st], c->cls_ptr[st + 1]);
    for (int i = 0; i < m; ++i)
        if (pr->i_k[i] < c->cls_ptr[t->stage[i]] || pr->i_k[i] >= c->cls_ptr[t->stage[i] + 1])
            return fail(RAOCP_ERR_ARG, "classes must be numbered by stage");
    c->pair_ptr.assign(nk + 1, (int)pairs.size());
    for (int q = (int)pairs.size() - 1; q >= 0; --q) c->pair_ptr[pairs[q].second] = q;
    for (int c_ = nk - 1; c_ >= 0; --c_) c->pair_ptr[c_] = std::min(c->pair_ptr[c_], c->pair_ptr[c_ + 1]);
    c->nkind = (int)kinds.size();
    D.nkind = c->nkind;
    std::vector<double>&W = dt.W, &RG = dt.RG, &KM = dt.KM, &F = dt.F, &WT = dt.WT;
    W.assign(std::max<size_t>(1, kinds.size()) * R * SKP, 0.0);
    for (size_t q = 0; q < kinds.size(); ++q)
        for (int rho = 0; rho < R; ++rho)
            for (int k = 0; k < nx; ++k)
                W[(q * R + rho) * SKP + k] =
                    rho < nu ? Bm(kinds[q].second, k, rho) : A(kinds[q].first, k, rho - nu);  // B', A'
    RG.assign((size_t)nk * R * SNU, 0.0);
    KM.assign((size_t)nk * nu * SKP, 0.0);
    for (int c_ = 0; c_ < nk; ++c_) {
        for (int r = 0; r < nu; ++r) {
            for (int k = 0; k < nu; ++k) RG[((size_t)c_ * R + r) * SNU + k] = Ri(c_, r, k);
            for (int k = 0; k < nx; ++k) KM[((size_t)c_ * nu + r) * SKP + k] = K(c_, r, k);
        }
        for (int r = 0; r < nx; ++r)
            for (int k = 0; k < nu; ++k) {
                double g = 0.0;
                for (int t2 = 0; t2 < nu; ++t2) g += M(c_, r, t2) * Ri(c_, t2, k);
                RG[((size_t)c_ * R + nu + r) * SNU + k] = g - K(c_, k, r);
            }
    }
    F.assign(std::max<size_t>(1, pairs.size()) * nx * SKF, 0.0);
    for (size_t q = 0; q < pairs.size(); ++q) {
        const int ia = kinds[pairs[q].first].first, ib = kinds[pairs[q].first].second, c_ = pairs[q].second;
        for (int r = 0; r < nx; ++r) {
            for (int k = 0; k < nx; ++k) {
                double bk = 0.0;
                for (int t2 = 0; t2 < nu; ++t2) bk += Bm(ib, r, t2) * K(c_, t2, k);
                F[(q * nx + r) * SKF + k] = A(ia, r, k) + bk;  // Abar = A + B K (cache.py:226)
            }
            for (int k = 0; k < nu; ++k) F[(q * nx + r) * SKF + nx + k] = Bm(ib, r, k);
        }
    }
    // one-phase backward levels: WT[pair] = [-Rinv B' ; A' - G B'] of (child kind, parent class)
    WT.assign(std::max<size_t>(1, pairs.size()) * R * SKP, 0.0);
    for (size_t q = 0; q < pairs.size(); ++q) {
        const int ia = kinds[pairs[q].first].first, ib = kinds[pairs[q].first].second, c_ = pairs[q].second;
        for (int tr = 0; tr < R; ++tr)
            for (int k = 0; k < nx; ++k) {
                double v = 0.0;
                if (tr < nu) {
                    for (int t2 = 0; t2 < nu; ++t2) v -= Ri(c_, tr, t2) * Bm(ib, k, t2);
                } else {
                    const double* grow = &RG[((size_t)c_ * R + tr) * SNU];
                    for (int t2 = 0; t2 < nu; ++t2) v -= grow[t2] * Bm(ib, k, t2);
                    v += A(ia, k, tr - nu);
                }
                WT[(q * R + tr) * SKP + k] = v;
            }
    }
    if ((rc = c->upload_vec(&D.dW, W)) || (rc = c->upload_vec(&D.dRG, RG)) || (rc = c->upload_vec(&D.dKM, KM)) ||
        (rc = c->upload_vec(&D.dF, F)) || (rc = c->upload_vec(&D.dWT, WT)))
        return rc;
    return RAOCP_OK;
}

int setup_dyn3_dyn2(raocp_ctx* c, const raocp_tree_desc* t, const raocp_problem_desc* pr, const DynTables& dt) {
    const int n = c->n, m = c->m, nx = c->nx, nu = c->nu, N = c->N, nk = pr->n_k;
    const int R = dt.R, SKP = dt.SKP, SKF = dt.SKF, SNU = dt.SNU;
    int rc;
    const std::vector<int>&kind = dt.kind, &pair = dt.pair;
    const std::vector<std::pair<int, int>>&kinds = dt.kinds, &pairs = dt.pairs;
    const std::vector<double>&W = dt.W, &RG = dt.RG, &KM = dt.KM, &F = dt.F;
    // per-stage MFMA dynamics (raocp_dyn2.hip): column-major tables M[k R + r] and, per
    // stage, tiles of <= 16 nodes sharing a table (fp32 contexts; fp64 opt-in RAOCP_DYN2=1)
    c->dyn2 = c->f32 || env_flag("RAOCP_DYN2", false);
    {
        // the per-stage streaming sweep (raocp_dyn3.hip): one branching factor C <= 4, the
        // children's slot k of one kind at every parent of a stage, one class per stage, and
        // the compile-time sizes
        const int C = t->nch[0];
        // (fp64 at nx = 64: the stage's tables exceed the 160 KB of LDS)
        bool ok = C >= 1 && C <= 4 && ((nx == 20 && nu == 8) || (nx == 32 && nu == 12) || (nx == 64 && nu == 16)) &&
                  dyn3_lds_fits(c->f32, nx, nu, C);
        for (int i = 0; i < m && ok; ++i)
            if (t->nch[i] != C || t->ch_start[i] != 1 + C * i) ok = false;
        std::vector<raocp::Dy3Stage> sts;
        for (int st = 0; st < N && ok; ++st) {
            raocp::Dy3Stage d{};
            d.i0 = c->stage_ptr[st];
            d.i1 = c->stage_ptr[st + 1];
            d.leaf = st + 1 == N;
            d.cls = pr->i_k[d.i0];
            for (int k = 0; k < 4; ++k) {
                d.kind[k] = k < C ? kind[1 + C * d.i0 + k] : 0;
                d.pair[k] = k < C ? pair[1 + C * d.i0 + k] : 0;
            }
            for (int i = d.i0; i < d.i1 && ok; ++i) {
                if (pr->i_k[i] != d.cls) ok = false;
                for (int k = 0; k < C && ok; ++k)
                    if (kind[1 + C * i + k] != d.kind[k] || pair[1 + C * i + k] != d.pair[k]) ok = false;
            }
            sts.push_back(d);
        }
        c->reg_ok = ok && C >= 2;
        c->reg_C = C;
        c->reg_st = sts;
        // default: fp32, and fp64 trees of >= 64k nodes (config 4: 118 vs 143 us for the
        // tiers; config 2 keeps the tiers, whose few launches win on small trees)
        c->dyn3 = ok && (c->f32 || n >= 65536);
        c->dyn3 = ok && env_flag("RAOCP_DYN3", c->dyn3);
        if (c->dyn3) {
            c->d3st = sts;
            c->dyn2 = false;
            c->unif_branch = C;
        }
    }
    if (c->dyn2 || c->dyn3) {
        const size_t nkd = std::max<size_t>(1, kinds.size()), npr = std::max<size_t>(1, pairs.size());
        std::vector<double> W2(nkd * R * nx, 0.0), RG2((size_t)std::max(1, nk) * R * nu, 0.0),
            KM2((size_t)std::max(1, nk) * nu * nx, 0.0), F2(npr * nx * (nx + nu), 0.0);
        for (size_t q = 0; q < kinds.size(); ++q)
            for (int r = 0; r < R; ++r)
                for (int k = 0; k < nx; ++k) W2[(q * nx + k) * R + r] = W[(q * R + r) * SKP + k];
        for (int c_ = 0; c_ < nk; ++c_) {
            for (int r = 0; r < R; ++r)
                for (int k = 0; k < nu; ++k) RG2[((size_t)c_ * nu + k) * R + r] = RG[((size_t)c_ * R + r) * SNU + k];
            for (int r = 0; r < nu; ++r)
                for (int k = 0; k < nx; ++k) KM2[((size_t)c_ * nx + k) * nu + r] = KM[((size_t)c_ * nu + r) * SKP + k];
        }
        for (size_t q = 0; q < pairs.size(); ++q)
            for (int r = 0; r < nx; ++r)
                for (int k = 0; k < nx + nu; ++k) F2[(q * (nx + nu) + k) * nx + r] = F[(q * nx + r) * SKF + k];
        if ((rc = upload_t(c, &c->W2, W2)) || (rc = upload_t(c, &c->RG2, RG2)) || (rc = upload_t(c, &c->KM2, KM2)) ||
            (rc = upload_t(c, &c->F2, F2)))
            return rc;
    }
    if (c->dyn3) {
        if ((rc = c->alloc(&c->Q2, (size_t)n * nx)) || (rc = c->alloc(&c->Dd2, (size_t)m * nu)) ||
            (rc = dyn3_images(c)))
            return rc;
        c->dyn32 = c->f32;
    }
    if (c->dyn2) {
        std::vector<int> idx;
        std::vector<raocp::DynTile> tl;
        // nodes [a, b) grouped by table (stable), cut into tiles of <= 16
        auto add = [&](int a, int b, auto table_of) {
            std::vector<std::pair<int, int>> it;
            for (int v = a; v < b; ++v) it.push_back({table_of(v), v});
            std::stable_sort(it.begin(), it.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
            for (size_t q = 0; q < it.size();) {
                size_t e = q;
                while (e < it.size() && e - q < 16 && it[e].first == it[q].first) ++e;
                tl.push_back(raocp::DynTile{(int)idx.size(), (int)(e - q), it[q].first, 0});
                for (size_t k = q; k < e; ++k) idx.push_back(it[k].second);
                q = e;
            }
        };
        c->d2_off.assign((size_t)N * 5, 0);
        for (int st = 0; st < N; ++st) {
            int* o = &c->d2_off[(size_t)st * 5];
            const int pb = c->stage_ptr[st], pe = c->stage_ptr[st + 1], cb_ = pe, ce_ = c->stage_ptr[st + 2];
            o[0] = (int)tl.size();
            add(cb_, ce_, [&](int j) { return kind[j]; });
            o[1] = (int)tl.size();
            add(pb, pe, [&](int i) { return pr->i_k[i]; });
            o[2] = (int)tl.size();
            add(pb, pe, [&](int i) { return pr->i_k[i]; });
            o[3] = (int)tl.size();
            add(cb_, ce_, [&](int j) { return pair[j]; });
            o[4] = (int)tl.size();
        }
        if ((rc = c->upload_vec(&c->d2_idx, idx)) || (rc = c->upload_vec(&c->d2_tiles, tl)) ||
            (rc = c->alloc(&c->Q2, (size_t)n * nx)) || (rc = c->alloc(&c->PA2, (size_t)n * R)) ||
            (rc = c->alloc(&c->Dd2, (size_t)m * nu)))
            return rc;
        c->dyn32 = c->f32;
    }
    return RAOCP_OK;
}

int setup_dr(raocp_ctx* c, const DynTables& dt, int n_cus) {
    const int nx = c->nx, nu = c->nu, N = c->N;
    // the regular-tree sweep (raocp_dynr.hip): fp64 regular trees of the compiled sizes
    c->dr = false;
    // (RAOCP_DYN3=1 / RAOCP_DYN2=1 keep the per-stage sweeps they ask for)
    if (c->reg_ok && !c->f32 && !c->dyn3 && !c->dyn2 && raocp::dr_supported(nx, nu, c->reg_C) && N >= 2) {
        if (env_flag("RAOCP_DR", true)) return dr_setup(c, dt, n_cus);
    }
    return RAOCP_OK;
}

int upload_node_records(raocp_ctx* c, const raocp_tree_desc* t, const raocp_problem_desc* pr, const DynTables& dt) {
    const int n = c->n, m = c->m, nx = c->nx, nu = c->nu, N = c->N;
    Dev& D = c->dev;
    int rc;
    const std::vector<int>&kind = dt.kind, &pair = dt.pair;
    std::vector<raocp::Rec> ninfo(m), cinfo(n);
    for (int i = 0; i < m; ++i) ninfo[i] = raocp::Rec{t->ch_start[i], t->nch[i], pr->i_k[i], t->stage[i]};
    cinfo[0] = raocp::Rec{0, 0, -1, 0};
    for (int j = 1; j < n; ++j) cinfo[j] = raocp::Rec{kind[j], pair[j], t->anc[j], 0};
    // CP child blocks (k_cp_dual): child records and each block's parent range
    {
        std::vector<raocp::Rec> crec(n, raocp::Rec{0, 0, 0, 0});
        for (int j = 1; j < n; ++j) crec[j] = raocp::Rec{t->anc[j], pr->i_sq[j], pr->i_sr[j], 0};
        const int per = kBlock / (nx + nu + 2);
        std::vector<raocp::Rec> dblk;
        for (int j0 = 1; j0 < n; j0 += per) {
            const int j1 = std::min(n, j0 + per), J = j1 - j0;
            const int a0 = t->anc[j0], a1 = t->anc[j1 - 1], na = a1 - a0 + 1;
            auto reg = [](int cnt) { return (cnt + 1) / 2 * 2 + 2; };
            const int need = 2 * reg(na * nx) + 2 * reg(na * nu) + 2 * reg(J) + reg(J * nx) + reg(J * nu) +
                             2 * reg(J) + reg(2 * J);
            if (need > raocp::kStageDual)
                return fail(RAOCP_ERR_ARG, "dual child block staging exceeds the LDS buffer");
            dblk.push_back(raocp::Rec{a0, a1, 0, 0});
        }
        if ((rc = c->upload_vec(&D.crec, crec)) || (rc = c->upload_vec(&D.dblk, dblk))) return rc;
    }
    if ((rc = c->upload_vec(&D.ninfo, ninfo)) || (rc = c->upload_vec(&D.cinfo, cinfo)) ||
        (rc = c->upload_vec(&D.stage_ptr, c->stage_ptr)))
        return rc;
    D.N = N;
    return RAOCP_OK;
}

// ---- dynamics plan (raocp_tierplan.h): the top's stages and the tiers below it, or per-stage
// launches when nothing fits; the workgroup sizes of its launches
raocp::TierSizes tier_sizes(const raocp_ctx* c, const DynTables& dt) {
    return raocp::TierSizes{c->nx, c->nu, c->KP, c->KF, c->NUP, c->PS, dt.SKP, dt.SKF, dt.SNU};
}
raocp::TierPlanResult plan_dyn_tiers(raocp_ctx* c, const raocp_tree_desc* t, const DynTables& dt, int n_cus) {
    // workgroup sizes (multiples of 64, at most 1024). The plan below is costed for
    // 1024-lane workgroups; launching its tiers with 512 lanes measured 98.0 vs 106.5 us
    // per CP iteration at config 2 and 577 vs 589 us at config 4 (more co-resident
    // workgroups per CU, cheaper barriers), while re-costing the plan for 512 or 256
    // lanes picked worse plans (config 4: 906 / 815 us). RAOCP_DYN_BLOCK /
    // RAOCP_DYN_TOP_BLOCK override.
    auto wg_env = [](const char* name, int def) {
        const int v = env_int(name, def);
        return v >= 64 && v <= 1024 && v % 64 == 0 ? v : def;
    };
    c->dyn_block = wg_env("RAOCP_DYN_BLOCK", 512);
    // the top on 512 lanes like the split sweep's top workgroups (kFuseBlock): the level
    // routines pick their split-k width from the lane count, so a sharded solve (tier
    // launches) reproduces the unsharded one (split sweep) bit for bit
    c->dyn_top_block = wg_env("RAOCP_DYN_TOP_BLOCK", raocp::kFuseBlock);
    if (dt.R * raocp::kKS > c->dyn_block) c->dyn_block = 1024;  // a child's split-k rows in one workgroup
    // fold: one-phase backward levels (per-pair WT tables instead of per-kind W, no P rows)
    // the default: config 2's split sweep 47.1 vs 49.5 us, the tier launches 51.4 vs 51.5 us
    // (profiles/r03_v5/dyn_time.log); RAOCP_DYN_FOLD=0 keeps the two-phase levels
    const bool fold_ok = env_flag("RAOCP_DYN_FOLD", true);
    const char* env = getenv("RAOCP_DYN_PER_STAGE");
    const raocp::TierTree tr{c->n, c->N, c->stage_ptr.data(), t->ch_start, t->nch, c->cls_ptr.data(), c->pair_ptr.data(), c->nkind};
    return raocp::plan_tiers(tr, tier_sizes(c, dt), raocp::TierLimits{raocp::kMaxLevels, raocp::kMaxTopStages}, n_cus,
                             fold_ok, env && env[0] == '1');
}

// the plan on the context: per tier its level ranges and the kernel argument of a regular tier
int build_tier_plans(raocp_ctx* c, const raocp_tree_desc* t, const raocp::TierPlanResult& plan) {
    int rc;
    c->cut = plan.cut;
    c->lds_top = plan.lds_top;
    c->maxch_top = plan.maxch_top;
    c->f_lds_top = plan.f_lds_top;
    c->fold_top = plan.fold_top;
    for (const raocp::TierCut& w : plan.tiers) {
        const int a = w.s0, b = w.s1, L = b - a;
        raocp_ctx::TierPlan tp;
        tp.s0 = a;
        tp.s1 = b;
        tp.nsub = c->stage_ptr[a + 1] - c->stage_ptr[a];
        tp.maxch = w.maxch;
        tp.lds_b = w.lds_b;
        tp.lds_f = w.lds_f;
        tp.fm = w.fm;
        tp.fold = w.fold;
        std::vector<raocp::Rec> lv;  // level ranges {lo, hi, off} of every subtree of the tier
        for (int r = c->stage_ptr[a]; r < c->stage_ptr[a + 1]; ++r) {
            int lo = r, hi = r + 1, acc = 0;
            for (int l = 0; l <= L; ++l) {
                lv.push_back(raocp::Rec{lo, hi, acc, 0});
                acc += hi - lo;
                if (l < L) {
                    const int nlo = t->ch_start[lo], nhi = t->ch_start[hi - 1] + t->nch[hi - 1];
                    lo = nlo;
                    hi = nhi;
                }
            }
        }
        if ((rc = c->upload_vec(&tp.lv, lv))) return rc;
        // regular tier: every subtree has the same level sizes and consecutive ids
        memset(&tp.ta, 0, sizeof(tp.ta));
        for (int l = 0; l <= L; ++l) tp.ta.pl0[l] = c->pair_ptr[c->cls_ptr[a + l]];
        tp.ta.regular = 1;
        for (int l = 0; l <= L; ++l) {
            tp.ta.lo0[l] = lv[l].x;
            tp.ta.cnt[l] = lv[l].y - lv[l].x;
        }
        for (int r = 0; r < tp.nsub && tp.ta.regular; ++r)
            for (int l = 0; l <= L; ++l) {
                const raocp::Rec& e = lv[(size_t)r * (L + 1) + l];
                if (e.x != tp.ta.lo0[l] + r * tp.ta.cnt[l] || e.y - e.x != tp.ta.cnt[l]) {
                    tp.ta.regular = 0;
                    break;
                }
            }
        c->tiers.push_back(tp);
    }
    return RAOCP_OK;
}

// ---- the split sweep (raocp_dynf.hip): the same tiers in TWO launches, one workgroup
// per subtree of every tier plus the top, for regular tiers of >= 2 subtrees per parent
// subtree with the top's F in LDS (RAOCP_DYN_SPLIT=0 keeps the tier launches). Its
// waits are for workgroups of the same launch, so it runs only where the whole grid is
// co-resident (the occupancy query): no wait then depends on the dispatch order.
int setup_split_sweep(raocp_ctx* c, const DynTables& dt, int n_cus) {
    const int nx = c->nx, nu = c->nu, KP = c->KP, KF = c->KF, NUP = c->NUP, PS = c->PS;
    const raocp::TierTabs tb = raocp::tier_tabs(tier_sizes(c, dt));
    const size_t kLds = raocp::kTierLds, W1 = tb.W1, RG1 = tb.RG1, KM1 = tb.KM1, F1 = tb.F1;
    const std::vector<int>&cp = c->cls_ptr, &pp = c->pair_ptr;
    auto stage_n = [&](int st) { return c->stage_ptr[st + 1] - c->stage_ptr[st]; };
    auto recs = [](size_t cnt) { return raocp::tier_recs(cnt); };
    int rc;
    c->dyn_split = false;
    bool fz = c->cut > 0 && !c->tiers.empty() && c->tiers.size() <= (size_t)raocp::kFuseTiers && c->f_lds_top;
    bool split = env_flag("RAOCP_DYN_SPLIT", true);
    size_t up = 0, down = 0;  // doubles
    raocp::FuseArg& fa = c->fuse;
    memset(&fa, 0, sizeof(fa));
    for (size_t k = 0; fz && k < c->tiers.size(); ++k) {
        const auto& tp = c->tiers[k];
        const int L = tp.s1 - tp.s0;
        const int above = k == 0 ? 1 : c->tiers[k - 1].nsub;
        const int r = tp.nsub / above;
        const int per_parent = k == 0 ? stage_n(c->cut) : c->tiers[k - 1].ta.cnt[c->tiers[k - 1].s1 - c->tiers[k - 1].s0];
        fz = fz && tp.ta.regular && tp.fm != 0 && r >= 2 && r * above == tp.nsub && r == per_parent;
        if (!fz) break;
        raocp::FuseTier& ft = fa.t[k];
        size_t nnl = 0;
        for (int l = 0; l < L; ++l) nnl += tp.ta.cnt[l];
        const size_t nall = nnl + tp.ta.cnt[L];
        const int c0 = cp[tp.s0], c1 = cp[tp.s1], p0 = pp[c0], p1 = pp[c1];
        size_t npl = p1 - p0;
        if (tp.fm == 2) {
            npl = 0;
            for (int l = 0; l < L; ++l) npl = std::max<size_t>(npl, tp.ta.pl0[l + 1] - tp.ta.pl0[l]);
        }
        ft.s0 = tp.s0;
        ft.s1 = tp.s1;
        ft.r = r;
        ft.c0 = c0;
        ft.c1 = c1;
        ft.p0 = p0;
        ft.p1 = p1;
        ft.maxch = tp.maxch;
        ft.fm = tp.fm;
        ft.fold = tp.fold;
        ft.nnl = (int)nnl;
        ft.ngroups = above;
        ft.ta = tp.ta;
        ft.ta.boff = 0;
        const size_t back = (tp.fold ? (size_t)(p1 - p0) * W1 : c->nkind * W1) + (c1 - c0) * RG1 + nall * KP +
                            nnl * NUP + (tp.fold ? 0 : raocp::rup(tp.maxch * PS, 2)) + recs(nnl + nall - 1);
        const size_t fwd = (c1 - c0) * KM1 + npl * F1 + recs(nnl + nall - 1);
        up = std::max(up, back);
        down = std::max(down, (size_t)raocp::rup((int)(nnl * KF), 2) + fwd);
    }
    if (fz) {  // the top's backward (k_dyn_up) and forward (k_dyn_down) layouts
        const size_t T = c->stage_ptr[c->cut], nb = stage_n(c->cut);
        const int c1 = cp[c->cut], p1 = pp[c1];
        up = std::max(up, (c->fold_top ? (size_t)p1 * W1 : c->nkind * W1) + c1 * RG1 + T * KP + nb * KP + T * NUP +
                              T * KF + (c->fold_top ? 0 : raocp::rup(c->maxch_top * PS, 2)) + recs(T + T + nb - 1));
        down = std::max(down, c1 * KM1 + (c->f_lds_top ? (size_t)p1 * F1 : 0) + T * KF + recs(T + T + nb - 1));
        c->lds_up = 8 * up;
        c->lds_down = 8 * down;
        split = split && c->lds_up <= kLds && c->lds_down <= kLds;
    }
    if (fz && split) {
        fa.K = (int)c->tiers.size();
        long grid = 2;  // the top and the deferred stopping test's workgroup
        for (const auto& tp : c->tiers) grid += tp.nsub;
        int pu = 0, pd = 0;
        dispatch(nx, nu, SplitOcc{}, c, &pu, &pd);
        c->dyn_split = pu > 0 && pd > 0 && grid <= (long)n_cus * std::min(pu, pd);
    }
    if (c->dyn_split) {
        size_t words = 2;
        for (int k = 0; k < fa.K; ++k) words += 2 * (size_t)fa.t[k].ngroups;
        if ((rc = c->alloc(&c->fuse_sync, words))) return rc;
        if (hipMemset(c->fuse_sync, 0, words * sizeof(unsigned)) != hipSuccess)
            return fail(RAOCP_ERR_HIP, "hipMemset failed");
        c->fuse_words = words;
        fa.epoch = c->fuse_sync;
        fa.err = (int*)(c->fuse_sync + 1);
        unsigned* w = c->fuse_sync + 2;
        for (int k = 0; k < fa.K; ++k) {
            fa.t[k].cnt = w;
            fa.t[k].flag = w + fa.t[k].ngroups;
            w += 2 * (size_t)fa.t[k].ngroups;
        }
        fa.s = c->cut;
        fa.T = c->stage_ptr[c->cut];
        fa.nb = stage_n(c->cut);
        fa.c1 = cp[c->cut];
        fa.p1 = pp[fa.c1];
        fa.maxch_top = c->maxch_top;
        fa.fold_top = c->fold_top;
        fa.timeout = fuse_timeout_ticks();
    }
    return RAOCP_OK;
}

// ---- node-block CP kernels (raocp_cp.hip): records, block tables, block sizes
int setup_cp_blocks(raocp_ctx* c, const raocp_tree_desc* t, const raocp_problem_desc* pr, const Layout& lay) {
    const int n = c->n, m = c->m, nx = c->nx, nu = c->nu, cmax = c->cmax;
    Dev& D = c->dev;
    int rc;
    const std::vector<int>&yrel = lay.yrel, &e7off = lay.e7off, &e14off = lay.e14off;
    std::vector<int>& pos7 = c->h_pos7;
    std::vector<int>& pos14 = c->h_pos14;
    pos7.assign(m + 1, 0);
    pos14.assign(n - m + 1, 0);
    {
        int o = D.E7;
        for (int i = 0; i < m; ++i) { pos7[i] = o; o += e7off[i] >= 0 ? nx + nu : 1; }
        pos7[m] = o;
        o = D.E14 + m;  // the E14 segment has one placeholder per nonleaf node first
        for (int l = m; l < n; ++l) { pos14[l - m] = o; o += e14off[l - m] >= 0 ? nx : 1; }
        pos14[n - m] = o;
    }
    c->h_yrel = yrel;
    c->h_chs.assign(t->ch_start, t->ch_start + m);
    c->h_nch.assign(t->nch, t->nch + m);
    c->h_isq.assign(pr->i_sq, pr->i_sq + n);
    c->h_isr.assign(pr->i_sr, pr->i_sr + n);
    c->h_isp.assign(pr->i_sp, pr->i_sp + n);
    c->n_sq = pr->n_sq;
    c->n_sr = pr->n_sr;
    c->n_sp = pr->n_sp;
    std::vector<raocp::Rec> frec(m), lrec(n - m);
    for (int i = 0; i < m; ++i) frec[i] = raocp::Rec{yrel[i], t->nch[i], t->ch_start[i], e7off[i]};
    for (int l = m; l < n; ++l) lrec[l - m] = raocp::Rec{pr->i_sp[l], pr->i_box_l[l] >= 0 ? pr->i_box_l[l] : 0, e14off[l - m], 0};
    D.nBnl = c->nbn;
    D.nBl = c->nbl;
    if ((rc = c->upload_vec(&D.frec, frec)) || (rc = c->upload_vec(&D.lrec, lrec))) return rc;
    // block sizes: about 256 family and 256 leaf blocks, within the LDS budget
    const long kCpLds = 64 * 1024 / 8;  // doubles: keeps >= 2 blocks per CU
    // family blocks of one k_cpp lane chunk (kBlock / (nx + nu + cmax + 1) parents: the
    // chunks of a block run one after the other; measured +3.7 % it/s at config 2 over
    // 256 blocks of 16 parents), leaf blocks of ~1/256 of the leaves
    int FB = std::max(1, std::min((m + 255) / 256, kBlock / (nx + nu + cmax + 1))),
        LB = std::max(1, (n - m + 255) / 256);
    const std::vector<std::pair<int, int>> allp{{0, m}}, alll{{m, n}};
    while (FB > 1 && cp_need(c, allp, {}, FB, LB) > kCpLds) FB = FB * 3 / 4;
    while (LB > 1 && cp_need(c, {}, alll, FB, LB) > kCpLds) LB = LB * 3 / 4;
    c->cp_FB = FB;
    c->cp_LB = LB;
    // MFMA CP kernels: W waves per block, one 16-node tile per wave and pass; W from the
    // tile count (about two blocks per CU), at least the lanes of a parent-row group
    // (nx <= 64 and nu <= 32: validate_tree)
    {
        // four waves per block measured faster than one or two at configs 2 and 4 (the
        // per-block gather and barriers amortise over more tiles)
        int W = 4;
        const int lanes = std::max(2 * cmax + 2 + nx + nu, cmax + 1);
        W = std::max(W, (lanes + 63) / 64);
        if (W > 4) return fail(RAOCP_ERR_ARG, "parent rows exceed a 256-lane CP block (branching too large)");
        const double cavg = (double)(n - 1) / m;
        c->cp2_W = W;
        c->cp2_FB = std::max(1, (int)(16.0 * W / cavg + 1e-9));
        c->cp2_LB = 16 * W;
        // within 64 KB of LDS per block (two blocks per CU)
        const long kLds2 = 64 * 1024;
        while (c->cp2_FB > 1 && cp2_need(c, 0, m, c->cp2_FB, true) > kLds2)
            c->cp2_FB = std::min(c->cp2_FB - 1, c->cp2_FB * 3 / 4);
        while (c->cp2_LB > 1 && cp2_need(c, m, n, c->cp2_LB, false) > kLds2)
            c->cp2_LB = std::min(c->cp2_LB - 1, c->cp2_LB * 3 / 4);
        // small trees (config 2: 8,191 nodes, ~770 tiles) run the scalar kernels, which
        // spread a latency-bound launch over more lanes (measured 17.0 / 21.1 us vs 21.3 /
        // 23.6 us for k_cpd / k_cpp); from ~4k tiles the MFMA kernels win (config 4:
        // 200 / 196 us vs 210 / 318 us; config 3 464 vs 505 us per iteration)
        c->cp_v1 = (long)(n - 1 + 15) / 16 + (long)(n - m + 15) / 16 < 4096;
        if (c->f32) c->cp_v1 = false;  // fp32: the MFMA kernels unless blocks mix weight tables
        c->cp_v1 = env_flag("RAOCP_CP_V1", c->cp_v1);
    }
    return build_cp_blocks(c, allp, alll);
}

// ---- L / L^T node-range blocks (raocp_ell.hip): nonleaf and leaf ranges split evenly
// over B blocks; B from the node count (64 nodes per block), raised until every block's LDS stage fits 64 KB
int setup_ell_blocks(raocp_ctx* c, const raocp_tree_desc* t, const raocp_problem_desc* pr) {
    const int n = c->n, m = c->m, nx = c->nx, nu = c->nu;
    const std::vector<int>& yrel = c->h_yrel;
    int rc;
    // measured (round-2 A/B of the block size): 512-thread blocks while the grid is one block per CU,
    // 256-thread blocks of 64 nodes once there are several per CU
    int per = 64;
    int thr = (n + per - 1) / per > 512 ? 256 : 512;
    c->ell_threads = thr;
    const int Bmax = std::max(1, std::max(m, n - m));
    int B = std::max(1, std::min(std::max(256, (n + per - 1) / per), Bmax));
    std::vector<raocp::Rec> tab;
    long need_l = 0, need_t = 0;
    // LDS doubles of one gathered range (raocp_ell.hip Gather): 16-B chunks, +1 for a
    // range that starts 8 B into its first chunk
    auto dbl = [](long cnt) { return 2 * ((cnt * 8 + 15) / 16 + 1); };
    auto rec = [](long cnt) { return 2 * cnt + 2; };
    for (;;) {
        tab.assign((size_t)B * raocp::kEllRecs, raocp::Rec{0, 0, 0, 0});
        need_l = need_t = 0;
        for (int b = 0; b < B; ++b) {
            raocp::Rec* T = tab.data() + (size_t)b * raocp::kEllRecs;
            const int i0 = (int)((int64_t)b * m / B), i1 = (int)((int64_t)(b + 1) * m / B);
            const int l0 = m + (int)((int64_t)b * (n - m) / B), l1 = m + (int)((int64_t)(b + 1) * (n - m) / B);
            int c0 = 0, c1 = 0, y0 = 0, y1 = 0;
            if (i1 > i0) {
                c0 = t->ch_start[i0];
                c1 = t->ch_start[i1 - 1] + t->nch[i1 - 1];
                y0 = yrel[i0];
                y1 = yrel[i1 - 1] + 2 * t->nch[i1 - 1] + 1;
            }
            const int e7a = c->h_pos7[i0], e7b = c->h_pos7[i1];
            const int e14a = c->h_pos14[l0 - m], e14b = c->h_pos14[l1 - m];
            T[0] = raocp::Rec{i0, i1, c0, c1};
            T[1] = raocp::Rec{l0, l1, y0, y1};
            T[2] = raocp::Rec{e7a, e7b, e14a, e14b};
            // the block's table index of each product family, -1 when its nodes differ
            auto uni = [](const int* idx, int a, int b) {
                if (b <= a) return -1;
                for (int q = a + 1; q < b; ++q)
                    if (idx[q] != idx[a]) return -1;
                return idx[a];
            };
            // regular block (k_ell_t's per-parent MFMA tiles): every parent has the same
            // child count c <= 4 and its children are c0 + (i - i0) c + [0, c)
            int creg = 0;
            if (i1 > i0 && t->nch[i0] >= 1 && t->nch[i0] <= 4) {
                creg = t->nch[i0];
                for (int q = i0; q < i1 && creg; ++q)
                    if (t->nch[q] != creg || t->ch_start[q] != c0 + (q - i0) * creg) creg = 0;
            }
            T[3] = raocp::Rec{uni(pr->i_sq, c0, c1), uni(pr->i_sr, c0, c1), uni(pr->i_sp, l0, l1), creg};
            const long np = i1 - i0, nc = c1 - c0, nl = l1 - l0, Y = y1 - y0;
            need_l = std::max(need_l, dbl(np * nx) + dbl(np * nu) + dbl(Y) + dbl(np) + 2 * dbl(nc) + rec(np) +
                                          rec(nc) + dbl(nl * nx) + dbl(nl) + rec(nl));
            need_t = std::max(need_t, dbl(nc * nx) + dbl(nc * nu) + dbl(e7b - e7a) + dbl(Y) + dbl(np) +
                                          3 * dbl(nc) + rec(np) + rec(nc) + dbl(nl * nx) + dbl(e14b - e14a) +
                                          2 * dbl(nl) + rec(nl) + nc * (nx + nu));
        }
        if (std::max(need_l, need_t) * 8 <= 64 * 1024 || B >= Bmax) break;
        B = std::min(Bmax, B * 2);
    }
    if (std::max(need_l, need_t) * 8 > 64 * 1024)
        return fail(RAOCP_ERR_ARG, "L block does not fit LDS (node dimension too large)");
    if ((rc = c->upload_vec(&c->dev.ell_tab, tab))) return rc;
    c->ell_nb = B;
    c->ell_lds = need_l * 8;
    c->ellt_lds = need_t * 8;
    return RAOCP_OK;
}

// ---- iterate and work buffers
int alloc_iterate(raocp_ctx* c) {
    const int n = c->n, m = c->m, nx = c->nx, nu = c->nu, cmax = c->cmax;
    int rc;
    for (int b = 0; b < 3; ++b)
        if ((rc = c->alloc(&c->Z[b], c->P))) return rc;
    for (int b = 0; b < 2; ++b)
        if ((rc = c->alloc(&c->E[b], c->D))) return rc;
    if ((rc = c->alloc(&c->XI2, c->D)) || (rc = c->alloc(&c->q, (size_t)n * c->KP)) || (rc = c->alloc(&c->d, (size_t)m * nu + 2)) ||
        (rc = c->alloc(&c->gXQ, (size_t)n * c->KP)) || (rc = c->alloc(&c->gU, (size_t)m * c->NUP)) ||
        (rc = c->alloc(&c->gXD, (size_t)m * c->KF)) || (rc = c->alloc(&c->gP, (size_t)n * c->PS)) ||
        (rc = c->alloc(&c->x0, nx)) || (rc = c->alloc(&c->ctl, 1)) || (rc = c->alloc(&c->tmpP, c->P)) ||
        (rc = c->alloc(&c->tmpD, c->D)) || (rc = c->alloc(&c->part, 1024)) || (rc = c->alloc(&c->scal, 8)))
        return rc;
    if (hipHostMalloc((void**)&c->h_ctl, sizeof(Ctl), 0) != hipSuccess) return fail(RAOCP_ERR_HIP, "hipHostMalloc");
    if (hipHostMalloc((void**)&c->h_pub, sizeof(raocp::CtlPub), hipHostMallocCoherent) != hipSuccess ||
        hipHostGetDevicePointer((void**)&c->d_pub, c->h_pub, 0) != hipSuccess)
        return fail(RAOCP_ERR_HIP, "hipHostMalloc");
    memset(c->h_pub, 0, sizeof(raocp::CtlPub));
    {
        double* zp = nullptr;
        if ((rc = c->alloc(&zp, 16))) return rc;
        if (hipMemset(zp, 0, 16 * sizeof(double)) != hipSuccess) return fail(RAOCP_ERR_HIP, "memset");
        c->dev.zpage = zp;
    }
    {
        const int g_dual = groups(nx + nu + 2, n - 1).blocks + groups(2 * cmax + 2 + nx + nu, m).blocks +
                           groups(2 * nx + 2, n - m).blocks;
        const int g_primal = groups(nx + nu + cmax + 1, m).blocks + groups(nx, n - m).blocks;
        c->red_rows = std::max(std::max(g_dual, g_primal), std::max(c->cp_nbF + c->cp_nbL, c->cp2_nbF + c->cp2_nbL));
        if ((rc = c->alloc(&c->redpart, (size_t)c->red_rows * 6))) return rc;
        if (hipMemset(c->redpart, 0, (size_t)c->red_rows * 6 * sizeof(double)) != hipSuccess)
            return fail(RAOCP_ERR_HIP, "memset");
    }
    for (int b = 0; b < 3; ++b)
        if (hipMemset(c->Z[b], 0, c->P * sizeof(double)) != hipSuccess) return fail(RAOCP_ERR_HIP, "memset");
    for (int b = 0; b < 2; ++b)
        if (hipMemset(c->E[b], 0, c->D * sizeof(double)) != hipSuccess) return fail(RAOCP_ERR_HIP, "memset");
    if (hipMemset(c->XI2, 0, c->D * sizeof(double)) != hipSuccess || hipMemset(c->ctl, 0, sizeof(Ctl)) != hipSuccess ||
        hipMemset(c->q, 0, (size_t)n * c->KP * sizeof(double)) != hipSuccess ||
        hipMemset(c->gP, 0, (size_t)n * c->PS * sizeof(double)) != hipSuccess ||
        hipMemset(c->d, 0, (size_t)m * nu * sizeof(double)) != hipSuccess)
        return fail(RAOCP_ERR_HIP, "memset");
    c->bufs = raocp::Bufs{c->Z[0], c->Z[1], c->Z[2], c->E[0], c->E[1]};
    // RAOCP_EAGER=1: CP iterations launched one kernel at a time instead of the captured
    // graph (for rocprofv3 --kernel-trace --stats, which crashes replaying this graph)
    c->eager = env_flag("RAOCP_EAGER", c->eager);
    c->cur_z = c->Z[0];
    c->cur_e = c->E[0];
    c->dev.dyn_rot = 1;  // the tier kernels rotate the first wave of each staged range
    return ensure_hist(c, 1024);
}

// k_cp4: cp4_wpb waves per workgroup, the same waves over more CUs
int setup_cp4(raocp_ctx* c, long tiles) {
    c->cp4_wpb = env_flag("RAOCP_CP4_HELPER", c->cp4_wpb == 2) ? 2 : 1;
    c->cp3_grid = (int)std::max(1L, std::min(tiles, 8192L));  // one task per workgroup
    c->cp_rows = c->cp3_grid;
    return ensure_red_rows(c, c->cp3_grid);
}

int setup_cp6(raocp_ctx* c) {
    if (cp3_tasks(c->cp5_tk, {{c->cp3_mL, c->m}, {0, c->cp3_mL}}, 0, 0, 1, c->cp3_mL) < 0)
        return fail(RAOCP_ERR_ARG, "k_cp6 task list exceeds its parent-range slots");
    c->cp6_grid = raocp::cp6_grid(c->cp5_tk);
    c->cp6_grid = std::max(1, env_int("RAOCP_CP6_GRID", c->cp6_grid));
    c->cp_rows = raocp::cp6_rows(c->cp6_grid);
    return ensure_red_rows(c, c->cp_rows);
}

int setup_cp5(raocp_ctx* c) {
    const int n = c->n, m = c->m;
    if (cp3_tasks(c->cp5_tk, {{c->cp3_mL, m}, {0, c->cp3_mL}}, 0, 0, 1, c->cp3_mL) < 0)
        return fail(RAOCP_ERR_ARG, "k_cp5 task list exceeds its parent-range slots");
    // the leaf launch's form is read here, per context (a later context with another
    // RAOCP_CP5_LPF gets its own)
    c->cp5_lpf = env_flag("RAOCP_CP5_LPF", raocp::cp5_leaf_pf_default(c->f32));
    cp3_tasks(c->cp5_et, {{0, m}}, 0, 0, 1, 0, 64);
    c->cp5_gl = raocp::cp5_leaf_grid(c->cp5_et, m, n, c->cp5_lpf);
    // k_cp5_fams (profiles/r05/cp_time_fams*.log: config 4 100.7 -> 90.9 us, config 5
    // 335.3 -> 334.8 us, config 3 60.9 -> 57.4 us with the compacted slot sums)
    c->cp5_gf = raocp::cp5_fam_grid(c->cp5_tk);
    c->cp5_gl = std::max(1, env_int("RAOCP_CP5_LGRID", c->cp5_gl));
    c->cp5_gf = std::max(1, env_int("RAOCP_CP5_FGRID", c->cp5_gf));
    c->cp_rows = raocp::cp5_rows(c->cp5_gl, c->cp5_gf);
    return ensure_red_rows(c, c->cp_rows);
}

// the fused CP iteration's task list and weight image, and which of its forms runs
int setup_cp3(raocp_ctx* c) {
    const int n = c->n, m = c->m, nx = c->nx, nu = c->nu;
    int rc;
    c->cp3_mL = c->stage_ptr[c->N - 1];
    const long ptiles = (long)(m - c->cp3_mL + 15) / 16 + (c->cp3_mL + 15) / 16;
    // small trees (latency-bound: config 2 has 256 family tiles, one wave each) split
    // the leaves into tasks of their own: twice the waves, half the longest chain
    c->cp3_split = env_flag("RAOCP_CP3_SPLIT", ptiles < 1024);
    // leaf-parent tiles first (heavier), then the rest
    const long tiles = cp3_tasks(c->cp3_ta, {{c->cp3_mL, m}, {0, c->cp3_mL}}, m, c->cp3_split ? n : m,
                                 c->cp3_split, c->cp3_mL);
    if (tiles < 0) return fail(RAOCP_ERR_ARG, "k_cp3 task list exceeds its parent-range slots");
    c->cp3_grid = cp3_grid_of(tiles);
    if ((rc = ensure_red_rows(c, c->cp3_grid))) return rc;
    c->cp_rows = c->cp3_grid;
    if ((rc = cp3_image(c))) return rc;
    c->cp6 = raocp::cp6_supported(c->f32, nx, nu, c->unif_C, c->box_mode, c->dev.nBnl, c->dev.nBl);
    c->cp6 = c->cp6 && env_flag("RAOCP_CP6", true);
    c->cp4 = !c->cp6 && raocp::cp4_supported(c->f32, nx, nu, c->unif_C, c->box_mode);
    c->cp4 = c->cp4 && env_flag("RAOCP_CP4", true);
    if (c->cp4 && (rc = setup_cp4(c, tiles))) return rc;
    // k_cp5: the leaf tiles and the family tiles as two launches with small register
    // files (configs 3, 4, 5; k_cp4 keeps config 2)
    c->cp5 = !c->cp4 && !c->cp6 && raocp::cp5_supported(c->f32, nx, nu, c->unif_C, c->box_mode, c->dev.nBnl, c->dev.nBl);
    c->cp5 = c->cp5 && env_flag("RAOCP_CP5", true);
    if (c->cp6 && (rc = setup_cp6(c))) return rc;
    if (c->cp5 && (rc = setup_cp5(c))) return rc;
    return RAOCP_OK;
}

// ---- the streaming kernels: L / L^T (k_ell3 / k_ellt3), the box pattern they and the fused CP
// kernels share, and the fused CP iteration (setup_cp3)
int choose_streaming_kernels(raocp_ctx* c, const raocp_tree_desc* t, const raocp_problem_desc* pr) {
    const int n = c->n, m = c->m, nx = c->nx, nu = c->nu;
    // L by streaming wave tasks (raocp_ell3.hip): compile-time sizes, and one sqrtQ / sqrtR
    // table over all children and one sqrtPf over all leaves (the waves keep them in registers)
    bool uni = (nx == 20 && nu == 8) || (nx == 32 && nu == 12) || (nx == 64 && nu == 16);
    for (int j = 2; j < n && uni; ++j)
        if (pr->i_sq[j] != pr->i_sq[1] || pr->i_sr[j] != pr->i_sr[1]) uni = false;
    for (int l = m + 1; l < n && uni; ++l)
        if (pr->i_sp[l] != pr->i_sp[m]) uni = false;
    // measured (tools/ell3_check.py): config 2 fp64 4.9 vs 5.5 us, config 5 fp32 210 vs
    // 265 us, config 4 fp64 equal; RAOCP_ELL3=0 keeps the block kernels
    c->ell3 = uni && env_flag("RAOCP_ELL3", true);
    const long tasks = (long)(n - 1 + 15) / 16 + (n - m + 15) / 16 + ((long)m * (nx + nu) + (c->dev.T0 - c->dev.Y0) + m + 63) / 64;
    // grid sweep (profiles/r02_v2/ab_order.log): config 4 fp64 best at 2,048 blocks (25.3 us
    // vs 26.7 at 4,096), config 5 fp32 at 1,024 (116 vs 137 us at 4,096)
    c->ell3_grid = (int)std::max(1L, std::min((tasks + 3) / 4, c->f32 ? 1024L : 2048L));
    // L^T by streaming wave tasks: additionally one branching factor C <= 4 over all
    // nonleaf nodes (children 1 + C i .., y_i at (2C + 1) i); RAOCP_ELLT3=0 keeps k_ell_t
    int C = m > 0 ? t->nch[0] : 0;
    bool reg = uni && C >= 1 && C <= 4;
    for (int i = 0; i < m && reg; ++i)
        if (t->nch[i] != C || t->ch_start[i] != 1 + C * i) reg = false;
    c->unif_C = reg ? C : 0;
    {
        int nb = 0, lb = 0;
        for (int i = 0; i < m; ++i) nb += pr->i_box_nl[i] >= 0;
        for (int l = m; l < n; ++l) lb += pr->i_box_l[l] >= 0;
        c->box_mode = (nb == m ? 1 : nb == 0 ? 2 : 0) | ((lb == n - m ? 1 : lb == 0 ? 2 : 0) << 2);
        // RAOCP_BOX_MODE=0 forces the offset tables (always valid); any other value must
        // agree with the computed pattern (a forced "all boxed" on a tree with unboxed nodes
        // would compute eta7 / eta14 offsets for slots that do not exist)
        if (const char* e = getenv("RAOCP_BOX_MODE")) {
            const int v = atoi(e);
            if (v != 0 && v != c->box_mode)
                return fail(RAOCP_ERR_ARG, "RAOCP_BOX_MODE=" + std::to_string(v) + " disagrees with the tree's box "
                                                "pattern (" + std::to_string(c->box_mode) + "); only 0 may override");
            c->box_mode = v;
        }
    }
    reg = reg && env_flag("RAOCP_ELLT3", true);
    c->ellt3_C = reg ? C : 0;
    const long tasks_t = (long)(m + 4 * (4 / std::max(C, 1)) - 1) / (4 * (4 / std::max(C, 1))) + (n - m + 15) / 16 +
                         ((long)(c->dev.T0 - c->dev.Y0) + 2L * n - 1 + 63) / 64;
    // grid sweep (profiles/r02_v4/ab_grid.log): 1,536 blocks best at config 4 fp64 (24.0 us
    // vs 24.9 at 4,096, 28.0 at 1,024) and config 5 fp32 (109.4 vs 111.1 at 2,048)
    c->ellt3_grid = (int)std::max(1L, std::min((tasks_t + 3) / 4, 1536L));
    // the fused CP iteration (raocp_cp3.hip): uniform branching and tables (unif_C), the
    // compile-time sizes; RAOCP_CP3=0 keeps k_cpd* + k_cpp*
    c->cp3 = c->unif_C > 0 && c->ell3 && cp3_sizes(c->f32, nx, nu);
    c->cp3 = c->cp3 && env_flag("RAOCP_CP3", true);
    return c->cp3 ? setup_cp3(c) : RAOCP_OK;
}

}  // namespace
