// Stand-alone check of the forward map of the regular-tree sweep (csrc/raocp_drxfer.h, host
// only): random [Abar_k | B_k] and K per stage / slot of a binary tier with 4 levels at nx = 20,
// nu = 8, scaled to spectral norm <= 1, random x_0 and d rows. The level recursion
// x_(2n+1+k) = [Abar_k | B_k] [x_n ; d_n], u_n = K x_n + d_n in long double against the sweep
// from x_0 = 0 in double (the kernel's order: a 28-long dot as even and odd 16-B pairs over two
// accumulators) plus xf_apply_packed on the packed image.
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

// fwd_level's dot (raocp_dynr.hip): pairs p = 0, 2, .. into a, p = 1, 3, .. into b
static double dot_k(const double* w, const double* v, int n) {
    double a[2] = {0.0, 0.0}, b[2] = {0.0, 0.0};
    for (int p = 0; p < n / 2; ++p) {
        double* d = (p & 1) ? b : a;
        d[0] += w[2 * p] * v[2 * p];
        d[1] += w[2 * p + 1] * v[2 * p + 1];
    }
    return (a[0] + a[1]) + (b[0] + b[1]);
}

int main(int argc, char** argv) {
    const double bound = argc > 1 ? atof(argv[1]) : 1e-12;
    constexpr int nx = kXbNx, nu = kXbNu, R = nx + nu, NN = kXbNodes + kXbBnd;
    std::mt19937_64 rng(4321);
    std::normal_distribution<double> nd(0.0, 1.0);
    double worst = 0.0;
    for (int trial = 0; trial < 8; ++trial) {
        // trial 0 .. 5: norm <= 1 (1.0 / 1.001 of the estimate); 6, 7: contractions
        const double target = trial < 6 ? 1.0 : 0.5;
        std::vector<std::vector<double>> ab(kXbL * 2), km(kXbL), ku(kXbL);
        XfStages st;
        st.sab = R;
        st.skm = nx;
        auto fill = [&](std::vector<double>& m, int r, int c) {
            m.resize((size_t)r * c);
            for (double& v : m) v = nd(rng);
            const double s = spec_norm(m, r, c) * 1.001 / target;
            for (double& v : m) v /= s;
        };
        for (int l = 0; l < kXbL; ++l) {
            for (int k = 0; k < 2; ++k) {
                fill(ab[2 * l + k], nx, R);
                st.ab[l][k] = ab[2 * l + k].data();
            }
            fill(km[l], nu, nx);
            st.km[l] = km[l].data();
            // the kernel's u rows: [K row | unit vector]
            ku[l].assign((size_t)nu * R, 0.0);
            for (int i = 0; i < nu; ++i) {
                for (int j = 0; j < nx; ++j) ku[l][(size_t)i * R + j] = km[l][(size_t)i * nx + j];
                ku[l][(size_t)i * R + nx + i] = 1.0;
            }
        }
        std::vector<double> x0(nx), d((size_t)kXbNodes * nu);
        for (double& v : x0) v = nd(rng);
        for (double& v : d) v = nd(rng);
        // the level recursion in long double
        std::vector<long double> xr((size_t)NN * nx), ur((size_t)kXbNodes * nu);
        for (int j = 0; j < nx; ++j) xr[j] = x0[j];
        for (int n = 0; n < kXbNodes; ++n) {
            const int l = xb_level(n);
            for (int i = 0; i < nu; ++i) {
                long double s = d[(size_t)n * nu + i];
                for (int j = 0; j < nx; ++j) s += (long double)km[l][(size_t)i * nx + j] * xr[(size_t)n * nx + j];
                ur[(size_t)n * nu + i] = s;
            }
            for (int k = 0; k < 2; ++k)
                for (int i = 0; i < nx; ++i) {
                    long double s = 0.0L;
                    const double* row = &ab[2 * l + k][(size_t)i * R];
                    for (int j = 0; j < nx; ++j) s += (long double)row[j] * xr[(size_t)n * nx + j];
                    for (int j = 0; j < nu; ++j) s += (long double)row[nx + j] * d[(size_t)n * nu + j];
                    xr[(size_t)(2 * n + 1 + k) * nx + i] = s;
                }
        }
        // the sweep from x_0 = 0 in double, the kernel's order
        std::vector<double> xz((size_t)NN * nx, 0.0), uz((size_t)kXbNodes * nu);
        for (int n = 0; n < kXbNodes; ++n) {
            const int l = xb_level(n);
            double v[R];
            for (int j = 0; j < nx; ++j) v[j] = xz[(size_t)n * nx + j];
            for (int j = 0; j < nu; ++j) v[nx + j] = d[(size_t)n * nu + j];
            for (int i = 0; i < nu; ++i) uz[(size_t)n * nu + i] = dot_k(&ku[l][(size_t)i * R], v, R);
            for (int k = 0; k < 2; ++k)
                for (int i = 0; i < nx; ++i) xz[(size_t)(2 * n + 1 + k) * nx + i] = dot_k(&ab[2 * l + k][(size_t)i * R], v, R);
        }
        // plus the map's product with x_0 from its packed image
        const std::vector<double> M = xf_compose(st);
        std::vector<double> img(kDrXfN, 0.0);
        xf_pack(M, img.data());
        std::vector<double> io(kXfOut);
        for (int e = 0; e < kXbXn + kXbQn; ++e) io[e] = xz[nx + e];
        for (int e = 0; e < kXbUn; ++e) io[kXbXn + kXbQn + e] = uz[e];
        xf_apply_packed(img.data(), x0.data(), io.data());
        long double num = 0.0L, den = 0.0L;
        for (int e = 0; e < kXfOut; ++e) {
            const long double ref = e < kXbXn + kXbQn ? xr[nx + e] : ur[e - kXbXn - kXbQn];
            num = std::fmax(num, std::fabs((long double)io[e] - ref));
            den = std::fmax(den, std::fabs(ref));
        }
        const double rel = (double)(num / den);
        printf("trial %d (norm <= %.1f): x and u rows rel err %.3e\n", trial, target, rel);
        worst = std::fmax(worst, rel);
    }
    printf("worst rel err %.3e (bound %.1e)\n", worst, bound);
    return worst <= bound ? 0 : 1;
}
