// aa_host_main.cpp — host-only program over csrc/raocp_aa_ops.h (the regularised Cholesky solve of
// k_cpa) and csrc/raocp_cpa_layout.h (the acceleration's slab). Built by tests/test_accel_host.py
// with -fsanitize=address,undefined. Prints one line per check; exit code 1 when one fails.
//   solve:  random SPD systems G = M'M (M of 2j + 4 rows, so kappa(G) is of order 10) for
//           j = 1 .. 8 against the same algorithm in long double: forward error <= 1e-12
//           (kappa j eps ~ 1e-13) and backward error <= 1e-14 (|G||gamma| + |b|) (j eps ~ 1e-15)
//   refuse: an indefinite G, a zero G, a NaN in b, j = 0 and j = 9 return false
//   reginf: reg = +inf refuses for j = 1, 4 and 8, on an SPD G the default reg solves and on a zero G
//   layout: every array on 16 B, the stride on 256 B, no two arrays overlap, all inside the stride
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "raocp_aa_ops.h"
#include "raocp_cpa_layout.h"

using raocp::kAaMaxM;

static uint64_t g_s = 0x9e3779b97f4a7c15ull;
static double rnd() {  // uniform in (-1, 1)
    g_s = g_s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)((g_s >> 11) & ((1ull << 53) - 1)) / (double)(1ull << 52) - 1.0;
}

static bool ref_solve(int j, const double* G, const double* b, double reg, long double* gam) {
    long double L[kAaMaxM * kAaMaxM] = {0};
    long double tr = 0;
    for (int i = 0; i < j; ++i) tr += G[i * kAaMaxM + i];
    const long double shift = (long double)reg * (tr / j);
    for (int c = 0; c < j; ++c) {
        long double d = (long double)G[c * kAaMaxM + c] + shift;
        for (int k = 0; k < c; ++k) d -= L[c * kAaMaxM + k] * L[c * kAaMaxM + k];
        if (!(d > 0)) return false;
        L[c * kAaMaxM + c] = sqrtl(d);
        for (int i = c + 1; i < j; ++i) {
            long double s = G[i * kAaMaxM + c];
            for (int k = 0; k < c; ++k) s -= L[i * kAaMaxM + k] * L[c * kAaMaxM + k];
            L[i * kAaMaxM + c] = s / L[c * kAaMaxM + c];
        }
    }
    for (int i = 0; i < j; ++i) {
        long double s = b[i];
        for (int k = 0; k < i; ++k) s -= L[i * kAaMaxM + k] * gam[k];
        gam[i] = s / L[i * kAaMaxM + i];
    }
    for (int i = j - 1; i >= 0; --i) {
        long double s = gam[i];
        for (int k = i + 1; k < j; ++k) s -= L[k * kAaMaxM + i] * gam[k];
        gam[i] = s / L[i * kAaMaxM + i];
    }
    return true;
}

int main() {
    int bad = 0;
    const double reg = 1e-10;
    for (int j = 1; j <= kAaMaxM; ++j) {
        double worst_f = 0, worst_b = 0;
        for (int rep = 0; rep < 25; ++rep) {
            const int rows = 2 * j + 4;
            std::vector<double> M((size_t)rows * j);
            for (auto& v : M) v = rnd();
            double G[kAaMaxM * kAaMaxM] = {0}, Lw[kAaMaxM * kAaMaxM], b[kAaMaxM] = {0}, gam[kAaMaxM] = {0};
            for (int a = 0; a < j; ++a)
                for (int c = 0; c < j; ++c) {
                    double s = 0;
                    for (int r = 0; r < rows; ++r) s += M[(size_t)r * j + a] * M[(size_t)r * j + c];
                    G[a * kAaMaxM + c] = s;
                }
            for (int a = 0; a < j; ++a) b[a] = rnd();
            long double gr[kAaMaxM];
            if (!raocp::aa_solve(j, G, b, reg, gam, Lw) || !ref_solve(j, G, b, reg, gr)) {
                std::printf("solve j=%d rep=%d refused\n", j, rep);
                ++bad;
                continue;
            }
            long double tr = 0, en = 0, gn = 0, rn = 0, Gn = 0, bn = 0;
            for (int a = 0; a < j; ++a) tr += G[a * kAaMaxM + a];
            const long double shift = (long double)reg * (tr / j);
            for (int a = 0; a < j; ++a) {
                en += (gam[a] - gr[a]) * (gam[a] - gr[a]);
                gn += gr[a] * gr[a];
                bn += (long double)b[a] * b[a];
                long double s = -(long double)b[a];
                for (int c = 0; c < j; ++c) {
                    const long double g = (long double)G[a * kAaMaxM + c] + (a == c ? shift : 0);
                    s += g * gam[c];
                    Gn += g * g;
                }
                rn += s * s;
            }
            const double f = (double)(sqrtl(en) / sqrtl(gn));
            const double bw = (double)(sqrtl(rn) / (sqrtl(Gn) * sqrtl(gn) + sqrtl(bn)));
            worst_f = f > worst_f ? f : worst_f;
            worst_b = bw > worst_b ? bw : worst_b;
        }
        const bool ok = worst_f <= 1e-12 && worst_b <= 1e-14;
        std::printf("solve j=%d forward %.3e backward %.3e %s\n", j, worst_f, worst_b, ok ? "ok" : "FAIL");
        bad += !ok;
    }
    {
        double Lw[kAaMaxM * kAaMaxM], gam[kAaMaxM], b[kAaMaxM] = {1.0, 1.0};
        double G[kAaMaxM * kAaMaxM] = {0};
        G[0] = 1.0, G[1] = 2.0, G[kAaMaxM] = 2.0, G[kAaMaxM + 1] = 1.0;  // indefinite: second pivot 1 - 4
        const bool r1 = raocp::aa_solve(2, G, b, reg, gam, Lw);
        double Z[kAaMaxM * kAaMaxM] = {0};
        const bool r2 = raocp::aa_solve(3, Z, b, reg, gam, Lw);  // a zero pivot
        double I[kAaMaxM * kAaMaxM] = {0}, bn[kAaMaxM] = {1.0, std::nan("")};
        I[0] = I[kAaMaxM + 1] = 1.0;
        const bool r3 = raocp::aa_solve(2, I, bn, reg, gam, Lw);  // gamma not finite
        const bool r4 = raocp::aa_solve(0, I, b, reg, gam, Lw), r5 = raocp::aa_solve(kAaMaxM + 1, I, b, reg, gam, Lw);
        const bool r6 = raocp::aa_solve(2, I, b, reg, gam, Lw);  // and the identity is solved
        const bool ok = !r1 && !r2 && !r3 && !r4 && !r5 && r6 && std::fabs(gam[0] - 1.0 / (1.0 + reg)) <= 1e-15;
        std::printf("refuse indefinite=%d zero=%d nan=%d j0=%d j9=%d identity=%d %s\n", r1, r2, r3, r4, r5, r6, ok ? "ok" : "FAIL");
        bad += !ok;
    }
    {
        // reg = +inf: the shift is inf (tr > 0) or NaN (tr == 0), so the first pivot refuses
        const double inf = std::numeric_limits<double>::infinity();
        const int js[3] = {1, 4, kAaMaxM};
        bool r[3], z[3];
        for (int q = 0; q < 3; ++q) {
            const int j = js[q];
            double G[kAaMaxM * kAaMaxM] = {0}, Z[kAaMaxM * kAaMaxM] = {0}, Lw[kAaMaxM * kAaMaxM], b[kAaMaxM], gam[kAaMaxM];
            for (int a = 0; a < j; ++a) {
                b[a] = rnd();
                for (int c = 0; c <= a; ++c) G[a * kAaMaxM + c] = G[c * kAaMaxM + a] = (a == c ? 2.0 + j : 0.0) + 0.5 * rnd();
            }
            const bool solved = raocp::aa_solve(j, G, b, reg, gam, Lw);  // the same system is solved with the default
            r[q] = raocp::aa_solve(j, G, b, inf, gam, Lw) || !solved;
            z[q] = raocp::aa_solve(j, Z, b, inf, gam, Lw);  // tr = 0: inf * 0
        }
        const bool ok = !r[0] && !r[1] && !r[2] && !z[0] && !z[1] && !z[2];
        std::printf("reginf j1=%d j4=%d j8=%d zero1=%d zero4=%d zero8=%d %s\n", r[0], r[1], r[2], z[0], z[1], z[2], ok ? "ok" : "FAIL");
        bad += !ok;
    }
    {
        const long dims[][3] = {{380, 855, 5}, {380, 855, 1}, {380, 855, 8}, {599, 1308, 5}, {1, 1, 3}, {7, 12, 2}, {1001, 2002, 8}};
        bool ok = true;
        for (const auto& d : dims) {
            const raocp::CpaSlab L = raocp::cpa_layout_dims(d[0], d[1], (int)d[2]);
            const long m = d[2], st = (long)((sizeof(raocp::CpaState) + 7) / 8);
            const long beg[7] = {L.dg, L.dr, L.pg, L.pr, L.sg, L.G, L.state};
            const long len[7] = {m * L.vec, m * L.vec, L.vec, L.vec, L.vec, 64, st};
            ok = ok && L.vec >= d[0] + d[1] && L.vec % 2 == 0 && L.stride % 32 == 0 && L.m == m;
            for (int a = 0; a < 7; ++a) {
                ok = ok && beg[a] % 2 == 0 && beg[a] >= 0 && beg[a] + len[a] <= L.stride;
                for (int c = 0; c < a; ++c) ok = ok && (beg[c] + len[c] <= beg[a] || beg[a] + len[a] <= beg[c]);
            }
        }
        const raocp::CpaSlab Lm = raocp::cpa_layout_dims(380, 855, 5);
        std::printf("layout main m=5 stride %ld doubles %s\n", Lm.stride, ok ? "ok" : "FAIL");
        bad += !ok;
    }
    return bad ? 1 : 0;
}
