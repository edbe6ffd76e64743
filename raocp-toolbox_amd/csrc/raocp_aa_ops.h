// raocp_aa_ops.h — the small solver of the Anderson-accelerated batch kernel (k_cpa,
// raocp_cpb.hip) that a host program can run too: the regularised Cholesky solve of the
// least-squares normal equations, and the classification of one log record into the counters the
// accelerated step kernel keeps. No HIP runtime dependency: a plain host compiler takes this
// file (tests/accel/aa_host_main.cpp, tests/accel/aa_count_main.cpp).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RAOCP_AA_HD __host__ __device__ inline
#else
#define RAOCP_AA_HD inline
#endif

namespace raocp {

constexpr int kAaMaxM = 8;   // the largest memory (columns) of the acceleration
constexpr int kAaRec = 12;   // doubles of one log record: code, j, prop, |r|_2, gamma[8]

// What one log record adds to the four counters of a solve (k_mpc_step_aa, aa_counts of
// raocp_cp_batch_mpc_aa): cnt[0] proposals made (prop == 1), cnt[1] trials accepted (code == 2),
// cnt[2] trials rejected (code == 3), cnt[3] solves refused (prop == 2). A record may add to two of
// them: an accepted trial that goes on to propose or to a refused solve.
constexpr int kAaCounts = 4;
RAOCP_AA_HD void aa_count(int code, int prop, int* cnt) {
    cnt[0] += prop == 1 ? 1 : 0;
    cnt[1] += code == 2 ? 1 : 0;
    cnt[2] += code == 3 ? 1 : 0;
    cnt[3] += prop == 2 ? 1 : 0;
}

// gamma = (G + reg (tr G / j) I)^-1 b for the j <= kAaMaxM leading rows and columns of the
// symmetric G (row stride kAaMaxM; the lower triangle is read), by Cholesky, all in double.
// L is kAaMaxM x kAaMaxM doubles of work space. MP / VP are pointers to double in whatever
// address space the caller keeps them (the kernel: LDS). Returns false (gamma then holds nothing
// of use) when a pivot is not positive or not finite, or an entry of gamma is not finite.
// Every loop is bounded by j.
template <class MP, class VP>
RAOCP_AA_HD bool aa_solve(int j, MP G, VP b, double reg, VP gamma, MP L) {
    if (j < 1 || j > kAaMaxM) return false;
    double tr = 0.0;
    for (int i = 0; i < j; ++i) tr += G[i * kAaMaxM + i];
    const double shift = reg * (tr / (double)j);
    for (int c = 0; c < j; ++c) {
        double d = G[c * kAaMaxM + c] + shift;
        for (int k = 0; k < c; ++k) d -= L[c * kAaMaxM + k] * L[c * kAaMaxM + k];
        if (!(d > 0.0) || !(d <= 1.7976931348623157e308)) return false;
        const double dc = __builtin_sqrt(d);
        L[c * kAaMaxM + c] = dc;
        for (int i = c + 1; i < j; ++i) {
            double s = G[i * kAaMaxM + c];
            for (int k = 0; k < c; ++k) s -= L[i * kAaMaxM + k] * L[c * kAaMaxM + k];
            L[i * kAaMaxM + c] = s / dc;
        }
    }
    for (int i = 0; i < j; ++i) {  // L y = b
        double s = b[i];
        for (int k = 0; k < i; ++k) s -= L[i * kAaMaxM + k] * gamma[k];
        gamma[i] = s / L[i * kAaMaxM + i];
    }
    for (int i = j - 1; i >= 0; --i) {  // L' gamma = y
        double s = gamma[i];
        for (int k = i + 1; k < j; ++k) s -= L[k * kAaMaxM + i] * gamma[k];
        gamma[i] = s / L[i * kAaMaxM + i];
    }
    for (int i = 0; i < j; ++i)
        if (!(gamma[i] - gamma[i] == 0.0)) return false;  // NaN or infinite
    return true;
}

}  // namespace raocp
