// raocp_drxfer.h — composed maps of the regular-tree sweep (raocp_dynr.hip), host only: plain
// C++ with no HIP dependency (tests/test_dr_xfer_host.py compiles it with the host compiler).
//
// A tier of binary subtrees with 4 nonleaf levels (local BFS index n, children 2 n + 1 + k, the
// 16 boundary rows b below level 3; stage tables of level l: Phi_(l,k) = the lower nx rows of
// WT_k, RGq_l = the lower nx rows of RG). The backward recursion of the sweep,
//     q_n + x_n = RGq_l u_n + sum_k Phi_(l,k) q_(2n+1+k),
// is linear, so the one row a tier below the top owes its parent, its root's q row, is one
// product of the rows the subtree holds before its sweep: with P_0 = I and
// P_(2n+1+k) = P_n Phi_(lev(n),k),
//     q_0 + x_0 = sum_n P_n RGq_lev(n) u_n  -  sum_(n>=1) P_n x_n  +  sum_b P_b q_b.
// xb_compose builds that 20 x 720 map (long double accumulation, rounded once) over the inputs
// in the order [x of nodes 1..14 | q of the boundary rows 0..15 | u of nodes 0..14], xb_pack
// lays it out for the kernel: lane t = 24 r + c < 480 holds row r's entries [30 c, 30 c + 30)
// as 15 pairs, element-pair-major [pair p][lane][2] (every lane reads 16-B words, a wave's
// lanes adjacent ones). The forward sweep's map (xf_compose and its pack / apply) is at the end.
#pragma once

#include <cstddef>
#include <vector>

namespace raocp {

constexpr int kXbNx = 20, kXbNu = 8, kXbL = 4;
constexpr int kXbNodes = 15, kXbBnd = 16;                 // nonleaf nodes and boundary rows of a subtree
constexpr int kXbXn = (kXbNodes - 1) * kXbNx;             // 280: x of nodes 1..14
constexpr int kXbQn = kXbBnd * kXbNx;                     // 320: q of the boundary rows
constexpr int kXbUn = kXbNodes * kXbNu;                   // 120: u of nodes 0..14
constexpr int kXbIn = kXbXn + kXbQn + kXbUn;              // 720 inputs
constexpr int kXbChunks = 24, kXbPer = kXbIn / kXbChunks; // 24 chunks of 30 inputs per output row
constexpr int kXbPairs = kXbPer / 2;                      // 15 16-B words per lane
constexpr int kXbLanes = kXbNx * kXbChunks;               // 480 lanes
constexpr int kDrXbN = kXbPairs * kXbLanes * 2;           // doubles of a packed map
static_assert(kXbChunks * kXbPer == kXbIn && kXbPer % 2 == 0, "chunks of whole pairs");

// the tables of a tier's four stages: phi[l][k] points at Phi_(l,k) (nx x nx, row stride sphi),
// rgq[l] at RGq_l (nx x nu, row stride srg)
struct XbStages {
    const double* phi[kXbL][2];
    const double* rgq[kXbL];
    int sphi, srg;
};

inline int xb_level(int n) {
    int l = 0;
    for (int m = n + 1; m > 1; m >>= 1) ++l;
    return l;
}

// M (row-major 20 x 720): q_0 + x_0 = M [x_1..x_14 ; q_b0..q_b15 ; u_0..u_14]
inline std::vector<double> xb_compose(const XbStages& st) {
    constexpr int nx = kXbNx, nu = kXbNu;
    typedef long double ld;
    // P_n for the 15 nodes and the 16 boundary rows (index 15 + b)
    std::vector<std::vector<ld>> P(kXbNodes + kXbBnd, std::vector<ld>((size_t)nx * nx, 0.0L));
    for (int i = 0; i < nx; ++i) P[0][(size_t)i * nx + i] = 1.0L;
    for (int n = 0; n < kXbNodes; ++n) {
        const int l = xb_level(n);
        for (int k = 0; k < 2; ++k) {
            std::vector<ld>& c = P[2 * n + 1 + k];
            const double* f = st.phi[l][k];
            for (int i = 0; i < nx; ++i)
                for (int j = 0; j < nx; ++j) {
                    ld s = 0.0L;
                    for (int e = 0; e < nx; ++e) s += P[n][(size_t)i * nx + e] * (ld)f[(size_t)e * st.sphi + j];
                    c[(size_t)i * nx + j] = s;
                }
        }
    }
    std::vector<double> M((size_t)nx * kXbIn, 0.0);
    for (int i = 0; i < nx; ++i) {
        double* row = &M[(size_t)i * kXbIn];
        for (int n = 1; n < kXbNodes; ++n)
            for (int j = 0; j < nx; ++j) row[(n - 1) * nx + j] = (double)(-P[n][(size_t)i * nx + j]);
        for (int b = 0; b < kXbBnd; ++b)
            for (int j = 0; j < nx; ++j) row[kXbXn + b * nx + j] = (double)P[kXbNodes + b][(size_t)i * nx + j];
        for (int n = 0; n < kXbNodes; ++n) {
            const double* g = st.rgq[xb_level(n)];
            for (int j = 0; j < nu; ++j) {
                ld s = 0.0L;
                for (int e = 0; e < nx; ++e) s += P[n][(size_t)i * nx + e] * (ld)g[(size_t)e * st.srg + j];
                row[kXbXn + kXbQn + n * nu + j] = (double)s;
            }
        }
    }
    return M;
}

// the kernel's image of M: out[(p * 480 + t) * 2 + h] = M[r][30 c + 2 p + h], t = 24 r + c
inline void xb_pack(const std::vector<double>& M, double* out) {
    for (int r = 0; r < kXbNx; ++r)
        for (int c = 0; c < kXbChunks; ++c)
            for (int e = 0; e < kXbPer; ++e)
                out[((size_t)(e / 2) * kXbLanes + (r * kXbChunks + c)) * 2 + (e & 1)] = M[(size_t)r * kXbIn + c * kXbPer + e];
}

// The kernel's arithmetic on the host, in its order (the CPU test of the packed image): a lane's
// 15 pairs over two accumulators of two lanes each, the sum of a group of 8 lanes as three
// pairwise steps, a row's three group sums left to right; in: the 720 inputs, out: q_0 + x_0
inline void xb_apply_packed(const double* img, const double* in, double* out) {
    for (int r = 0; r < kXbNx; ++r) {
        double grp[kXbChunks / 8];
        for (int g = 0; g < kXbChunks / 8; ++g) {
            double v[8];
            for (int q = 0; q < 8; ++q) {
                const int c = 8 * g + q, t = r * kXbChunks + c;
                double a[2] = {0.0, 0.0}, b[2] = {0.0, 0.0};
                for (int p = 0; p < kXbPairs; ++p) {
                    const double* w = img + ((size_t)p * kXbLanes + t) * 2;
                    const double* x = in + c * kXbPer + 2 * p;
                    double* d = (p & 1) ? b : a;
                    d[0] += w[0] * x[0];
                    d[1] += w[1] * x[1];
                }
                v[q] = (a[0] + a[1]) + (b[0] + b[1]);
            }
            for (int q = 0; q < 8; q += 2) v[q] += v[q + 1];
            for (int q = 0; q < 8; q += 4) v[q] += v[q + 2];
            grp[g] = v[0] + v[4];
        }
        out[r] = (grp[0] + grp[1]) + grp[2];
    }
}

// ---- the forward sweep by superposition. The forward recursion x_(2n+1+k) = [Abar_k | B_k]
// [x_n ; d_n], u_n = K x_n + d_n is affine in the root's x row x_0: every row is its value in
// the sweep from x_0 = 0 (which needs the d rows only) plus a 20-long dot with x_0. With
// Psi_0 = I and Psi_(2n+1+k) = Abar_(lev(n),k) Psi_n the x row of node n gains Psi_n x_0 and its
// u row K_lev(n) Psi_n x_0. xf_compose builds that 720 x 20 map over the outputs in the order
// [x of nodes 1..14 | x of the boundary rows 0..15 | u of nodes 0..14] (long double
// accumulation, rounded once). The kernel adds it in two steps: first lane t < 512 one whole
// row (t < 320: boundary output t, so a tier above the deepest publishes them at once; t >= 320:
// output t - 320 of the other 400, "interior" = [x of nodes 1..14 | u]), then lane t < 416 half
// h = t % 2 (entries [10 h, 10 h + 10)) of interior output 192 + t / 2, the pair summed by DPP.
// xf_pack: [step 1: pair p < 10][lane < 512][2], then [step 2: pair p < 5][lane < 416][2].
constexpr int kXfOut = kXbXn + kXbQn + kXbUn;            // 720 outputs
constexpr int kXfInt = kXbXn + kXbUn;                    // 400 interior outputs
constexpr int kXfL1 = 512, kXfP1 = kXbNx / 2;            // step 1: lanes, 16-B words per lane
constexpr int kXfI1 = kXfL1 - kXbQn;                     // 192 interior outputs in step 1
constexpr int kXfL2 = 2 * (kXfInt - kXfI1), kXfP2 = kXbNx / 4;  // step 2: 416 lanes, 5 words
constexpr int kXfOff2 = kXfL1 * kXfP1 * 2;               // doubles of step 1's image
constexpr int kDrXfN = kXfOff2 + kXfL2 * kXfP2 * 2;      // doubles of a packed map
static_assert(kDrXfN == kXfOut * kXbNx && kXbNx % 4 == 0, "every entry of the map once");

// the forward tables of a tier's four stages: ab[l][k] points at [Abar_k | B_k] of stage l
// (nx rows, the first nx columns are Abar_k, row stride sab), km[l] at K_l (nu x nx, stride skm)
struct XfStages {
    const double* ab[kXbL][2];
    const double* km[kXbL];
    int sab, skm;
};

// output index of interior output i (x of nodes 1..14, then u)
inline int xf_interior(int i) { return i < kXbXn ? i : kXbXn + kXbQn + (i - kXbXn); }

// M (row-major 720 x 20): output e of the sweep gains M[e] . x_0
inline std::vector<double> xf_compose(const XfStages& st) {
    constexpr int nx = kXbNx, nu = kXbNu;
    typedef long double ld;
    std::vector<std::vector<ld>> P(kXbNodes + kXbBnd, std::vector<ld>((size_t)nx * nx, 0.0L));
    for (int i = 0; i < nx; ++i) P[0][(size_t)i * nx + i] = 1.0L;
    for (int n = 0; n < kXbNodes; ++n) {
        const int l = xb_level(n);
        for (int k = 0; k < 2; ++k) {
            std::vector<ld>& c = P[2 * n + 1 + k];
            const double* f = st.ab[l][k];
            for (int i = 0; i < nx; ++i)
                for (int j = 0; j < nx; ++j) {
                    ld s = 0.0L;
                    for (int e = 0; e < nx; ++e) s += (ld)f[(size_t)i * st.sab + e] * P[n][(size_t)e * nx + j];
                    c[(size_t)i * nx + j] = s;
                }
        }
    }
    std::vector<double> M((size_t)kXfOut * nx, 0.0);
    for (int n = 1; n < kXbNodes + kXbBnd; ++n)  // x rows: nodes 1..14, then the boundary (the same order)
        for (int e = 0; e < nx * nx; ++e) M[(size_t)(n - 1) * nx * nx + e] = (double)P[n][e];
    for (int n = 0; n < kXbNodes; ++n) {
        const double* g = st.km[xb_level(n)];
        for (int i = 0; i < nu; ++i)
            for (int j = 0; j < nx; ++j) {
                ld s = 0.0L;
                for (int e = 0; e < nx; ++e) s += (ld)g[(size_t)i * st.skm + e] * P[n][(size_t)e * nx + j];
                M[(size_t)(kXbXn + kXbQn + n * nu + i) * nx + j] = (double)s;
            }
    }
    return M;
}

// the kernel's image of M (kDrXfN doubles)
inline void xf_pack(const std::vector<double>& M, double* out) {
    for (int t = 0; t < kXfL1; ++t) {
        const int e = t < kXbQn ? kXbXn + t : xf_interior(t - kXbQn);
        for (int j = 0; j < kXbNx; ++j) out[((size_t)(j / 2) * kXfL1 + t) * 2 + (j & 1)] = M[(size_t)e * kXbNx + j];
    }
    for (int t = 0; t < kXfL2; ++t) {
        const int e = xf_interior(kXfI1 + t / 2), h = t & 1;
        for (int j = 0; j < kXbNx / 2; ++j)
            out[kXfOff2 + ((size_t)(j / 2) * kXfL2 + t) * 2 + (j & 1)] = M[(size_t)e * kXbNx + h * (kXbNx / 2) + j];
    }
}

// The kernel's arithmetic on the host, in its order: io holds the 720 outputs of the sweep from
// x_0 = 0 and gains the map's product with x0 in place. A lane's pairs go over two accumulators
// of two lanes each (even pairs, odd pairs), summed (a0 + a1) + (b0 + b1); step 2 adds its two
// halves, then the sum to the output.
inline void xf_apply_packed(const double* img, const double* x0, double* io) {
    auto dot = [&](const double* w, int stride, int pairs, const double* x) {
        double a[2] = {0.0, 0.0}, b[2] = {0.0, 0.0};
        for (int p = 0; p < pairs; ++p) {
            double* d = (p & 1) ? b : a;
            d[0] += w[(size_t)p * stride * 2] * x[2 * p];
            d[1] += w[(size_t)p * stride * 2 + 1] * x[2 * p + 1];
        }
        return (a[0] + a[1]) + (b[0] + b[1]);
    };
    for (int t = 0; t < kXfL1; ++t) {
        const int e = t < kXbQn ? kXbXn + t : xf_interior(t - kXbQn);
        io[e] += dot(img + 2 * t, kXfL1, kXfP1, x0);
    }
    for (int i = kXfI1; i < kXfInt; ++i) {
        const int t = 2 * (i - kXfI1);
        const double h0 = dot(img + kXfOff2 + 2 * t, kXfL2, kXfP2, x0);
        const double h1 = dot(img + kXfOff2 + 2 * (t + 1), kXfL2, kXfP2, x0 + kXbNx / 2);
        io[xf_interior(i)] += h0 + h1;
    }
}

}  // namespace raocp
