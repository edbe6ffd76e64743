// Stand-alone check of the composed maps of the regular-tree sweep (csrc/raocp_drxfer.h, host
// only): random stage matrices of a binary tier with 4 levels at nx = 20, nu = 8, scaled to
// spectral norm <= 1, the composed root map applied in the kernel's order from its packed image
// against the level recursion q_n + x_n = RGq u_n + sum_k Phi_k q_child(k) in long double.
// Prints the relative error of every trial; exit status 1 above the bound given as argv[1].
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "raocp_drxfer.h"

using namespace raocp;

// spectral norm of an r x c matrix (stride c) by power iteration on M'M
static double spec_norm(const std::vector<double>& M, int r, int c) {
    std::vector<double> v(c, 1.0), w(r);
    double s = 0.0;
    for (int it = 0; it < 200; ++it) {
        for (int i = 0; i < r; ++i) {
            w[i] = 0.0;
            for (int j = 0; j < c; ++j) w[i] += M[(size_t)i * c + j] * v[j];
        }
        double n = 0.0;
        for (int j = 0; j < c; ++j) {
            v[j] = 0.0;
            for (int i = 0; i < r; ++i) v[j] += M[(size_t)i * c + j] * w[i];
            n += v[j] * v[j];
        }
        n = std::sqrt(n);
        if (n == 0.0) return 0.0;
        for (int j = 0; j < c; ++j) v[j] /= n;
        s = std::sqrt(n);
    }
    return s;
}

int main(int argc, char** argv) {
    const double bound = argc > 1 ? atof(argv[1]) : 1e-12;
    constexpr int nx = kXbNx, nu = kXbNu;
    std::mt19937_64 rng(12345);
    std::normal_distribution<double> nd(0.0, 1.0);
    double worst = 0.0;
    for (int trial = 0; trial < 8; ++trial) {
        // trial 0 .. 5: norm exactly <= 1 (1.0 / 1.001 of the estimate); 6, 7: contractions
        const double target = trial < 6 ? 1.0 : 0.5;
        std::vector<std::vector<double>> phi(kXbL * 2), rgq(kXbL);
        XbStages st;
        st.sphi = nx;
        st.srg = nu;
        for (int l = 0; l < kXbL; ++l) {
            for (int k = 0; k < 2; ++k) {
                std::vector<double>& m = phi[2 * l + k];
                m.resize((size_t)nx * nx);
                for (double& v : m) v = nd(rng);
                const double s = spec_norm(m, nx, nx) * 1.001 / target;
                for (double& v : m) v /= s;
                st.phi[l][k] = m.data();
            }
            std::vector<double>& g = rgq[l];
            g.resize((size_t)nx * nu);
            for (double& v : g) v = nd(rng);
            const double s = spec_norm(g, nx, nu) * 1.001 / target;
            for (double& v : g) v /= s;
            st.rgq[l] = g.data();
        }
        // the rows of a subtree: x and u of the 15 nodes, q of the 16 boundary rows
        std::vector<double> x((size_t)kXbNodes * nx), u((size_t)kXbNodes * nu), qb((size_t)kXbBnd * nx);
        for (double& v : x) v = nd(rng);
        for (double& v : u) v = nd(rng);
        for (double& v : qb) v = nd(rng);
        // the level recursion in long double: q of every node, deepest level first
        std::vector<long double> q((size_t)(kXbNodes + kXbBnd) * nx);
        for (int b = 0; b < kXbBnd; ++b)
            for (int j = 0; j < nx; ++j) q[(size_t)(kXbNodes + b) * nx + j] = qb[(size_t)b * nx + j];
        for (int n = kXbNodes - 1; n >= 0; --n) {
            const int l = xb_level(n);
            for (int i = 0; i < nx; ++i) {
                long double s = 0.0L;
                for (int j = 0; j < nu; ++j) s += (long double)st.rgq[l][(size_t)i * nu + j] * u[(size_t)n * nu + j];
                for (int k = 0; k < 2; ++k)
                    for (int j = 0; j < nx; ++j)
                        s += (long double)st.phi[l][k][(size_t)i * nx + j] * q[(size_t)(2 * n + 1 + k) * nx + j];
                q[(size_t)n * nx + i] = s - (long double)x[(size_t)n * nx + i];
            }
        }
        // the composed map from its packed image, in the kernel's order
        const std::vector<double> M = xb_compose(st);
        std::vector<double> img(kDrXbN);
        xb_pack(M, img.data());
        std::vector<double> in(kXbIn), out(nx);
        for (int e = 0; e < kXbXn; ++e) in[e] = x[nx + e];
        for (int e = 0; e < kXbQn; ++e) in[kXbXn + e] = qb[e];
        for (int e = 0; e < kXbUn; ++e) in[kXbXn + kXbQn + e] = u[e];
        xb_apply_packed(img.data(), in.data(), out.data());
        long double num = 0.0L, den = 0.0L;
        for (int i = 0; i < nx; ++i) {
            const long double got = (long double)out[i] - (long double)x[i];  // q_0
            num = std::fmax(num, std::fabs(got - q[i]));
            den = std::fmax(den, std::fabs(q[i]));
        }
        const double rel = (double)(num / den);
        printf("trial %d (norm <= %.1f): root q row rel err %.3e\n", trial, target, rel);
        worst = std::fmax(worst, rel);
    }
    printf("worst rel err %.3e (bound %.1e)\n", worst, bound);
    return worst <= bound ? 0 : 1;
}
