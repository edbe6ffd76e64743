// raocp_cpb.hip — k_cpb: a BATCH of Chambolle–Pock solves on one small tree, as its own
// translation unit (host interface: raocp_cpb.h).
//
// The instances of a batch share the tree, every table and alpha; they differ in x0 (and in
// the starting iterate). ONE workgroup owns ONE instance and runs up to `chunk` whole CP
// iterations of it in one launch: nothing is handed from one workgroup to another (no flag,
// counter, spin or atomic between workgroups), every loop is bounded by `chunk`, a stage count
// or a row count, and the phases of an iteration are separated by workgroup barriers only.
//
// One iteration k, with p = Z[k % 3], z-half = Z[(k + 1) % 3] (already holding the half step
// z - alpha L^T eta with s_0 relaxed and (y, tau, s) projected on the AVaR kernel), d = E[k % 2]:
//   1. dynamics projection of (x, u) of Z[(k + 1) % 3] in place: backward over stages N-1..0
//      (child products [B'; A'] q_j, then d = Rinv v, q = (-x + a) + G v per node), forward
//      0..N-1 (u = K x + d, x_j = [Abar | B][x; d]); a barrier after every phase of a stage
//   2. dual half step v = (d + alpha L(2 z+ - p)) / alpha with the +-1/2 shifts  -> tv, and
//      L(z+ - p) -> xi2 (one lane per dual row)
//   3. prox of alpha g*: eta+ = alpha (v - Pi(v)) -> E[(k + 1) % 2], xi2, |xi2|, |delta2|
//   4. next half step Z[(k + 2) % 3] = z+ - alpha L^T eta+ (s_0 -= alpha, kernel projection)
//      together with xi0, xi1, delta0, delta1 of iteration k
//   5. the six NaN-propagating maxima of the workgroup, the history row and the stopping test
//      of cp_check_wave on the instance's own Ctl.
// The arithmetic of a row is that of the node-block kernels (raocp_cp.hip) and of the per-stage
// dynamics (raocp_dyn.hip: the same tables W, RG, KM, F of Dev with their padded row strides).
//
// Precision. The kernels are templates on the context's scalar type T (double or float): the
// slab, the tables and every row's FMA chain are T, nothing is promoted inside a row. An fp32
// context's tables are read as it holds them: Dev's L weights, box bounds, alpha_r and cond are
// floats there, and the dynamics tables are its column-major fp32 W2, RG2, KM2, F2 (CpbArg).
// The control block, the history rows, u0 and the records of k_mpc_step are double / int for
// either T (converted at the store); the stopping test compares in double.
//
// Memory. The instance's state (three primals, two duals, xi2, v, q, d, the child products)
// lives in its slab in HBM (CpbSlab); the slab of the main.py problem is a few KiB, so it stays
// in the L2 of the XCD the workgroup runs on. The tables every instance shares (sqrt Q, sqrt R,
// sqrt Pf, the box bounds) are staged in LDS once per launch when they fit kCpbLdsTabs.

#include "raocp_cpb.h"
#include "raocp_cpops.h"

namespace raocp {
namespace {

// explicit address spaces for either scalar type: global_load / ds_read, never flat
template <class T>
using gl = __attribute__((address_space(1))) T;
template <class T>
using cg = const __attribute__((address_space(1))) T*;
template <class T>
using cl = const __attribute__((address_space(3))) T*;
typedef __attribute__((address_space(1))) const int glbi;
template <class T>
using lds = __attribute__((address_space(3))) T;

constexpr __host__ __device__ int rup_(int a, int b) { return (a + b - 1) / b * b; }
// the row strides of the dynamics tables (raocp_common.h tstride)
constexpr __host__ __device__ int tstride_(int k) { return (k / 2) % 2 == 0 ? k + 2 : k; }

__device__ __forceinline__ int e3(const Dev& p, int j) { return p.E3 + 1 + (j - 1) * p.nx; }
__device__ __forceinline__ int e4(const Dev& p, int j) { return p.E4 + 1 + (j - 1) * p.nu; }
__device__ __forceinline__ int e11(const Dev& p, int l) { return p.E11 + p.m + (l - p.m) * p.nx; }

// (soc_apply, box_apply with the lane's NaN flag, nmx: raocp_cpops.h)

// the tables every instance shares, in LDS (PT = cl<T>) or in HBM (PT = cg<T>)
template <class PT>
struct Tabs {
    PT SQ, SR, SP, BLn, BHn, BLl, BHl;
};

// one instance's arrays for iteration k
template <class T>
struct View {
    gl<T>* pz;   // p = Z[k % 3]
    gl<T>* zp;   // z+ = Z[(k + 1) % 3]
    gl<T>* out;  // Z[(k + 2) % 3]
    gl<T>* d;    // E[k % 2]
    gl<T>* eo;   // eta+ = E[(k + 1) % 2]
    gl<T>* xi2;
    gl<T>* tv;
    gl<T>* q;
    gl<T>* dd;
    gl<T>* pb;
    cg<T> x0;
};

template <class T>
struct Maxima {
    T m0 = T(0), m1 = T(0), m2 = T(0), m3 = T(0), m4 = T(0), m5 = T(0);
    // one primal entry: pp = p, zz = z+, w = L^T(d - eta+), lc = L^T xi2
    __device__ __forceinline__ void account(T alpha, T pp, T zz, T w, T lc) {
        const T x1 = (pp - zz) / alpha - w;
        const T x0v = x1 + lc;
        const T dl1 = zz - pp;
        const T dl0 = dl1 + w;
        m0 = nmx<T>(m0, fabs(x0v));
        m1 = nmx<T>(m1, fabs(x1));
        m3 = nmx<T>(m3, fabs(dl0));
        m4 = nmx<T>(m4, fabs(dl1));
    }
};

// ---- the primal half step from the dual dA (FULL: eta+, with the residuals of the iteration;
// else the solve's first half step from d): src - alpha L^T dA, s_0 -= alpha, kernel projection
template <class T, bool FULL, class PT>
__device__ __forceinline__ void primal_phase(const Dev& p, const Tabs<PT>& tb, const View<T>& v, gl<T>* out, T alpha,
                                             Maxima<T>& mx, int tid, int nthr) {
    const int nx = p.nx, nu = p.nu, R = nx + nu;
    cg<T> pz = v.pz;
    cg<T> src = FULL ? v.zp : v.pz;
    cg<T> dA = FULL ? v.eo : v.d;
    cg<T> dP = v.d;
    cg<T> xg = v.xi2;
    glbrec* frec = (glbrec*)p.frec;
    glbrec* crec = (glbrec*)p.crec;
    glbrec* lrec = (glbrec*)p.lrec;
    // x / u rows of the nonleaf nodes: sum over children of sqrtQ_j eta3_j (sqrtR_j eta4_j) + eta7
    for (int it = tid; it < p.m * R; it += nthr) {
        const int i = it / R, r = it - i * R;
        const bool isx = r < nx;
        const int rr = isx ? r : r - nx;
        const Rec fr = frec[i];
        T accA = T(0), accW = T(0), accC = T(0);
        if (fr.w >= 0) {
            const int o = fr.w + r;
            accA = dA[o];
            if (FULL) {
                accW = dP[o] - dA[o];
                accC = xg[o];
            }
        }
        for (int q = 0; q < fr.y; ++q) {
            const int j = fr.z + q;
            const Rec cr = crec[j];
            const int len = isx ? nx : nu;
            const PT M = isx ? tb.SQ + (size_t)cr.y * nx * nx + rr : tb.SR + (size_t)cr.z * nu * nu + rr;
            const int o = isx ? e3(p, j) : e4(p, j);
            T sA = T(0), sW = T(0), sC = T(0);
            for (int k = 0; k < len; ++k) {
                const T mk = M[k * len], va = dA[o + k];
                sA = fma(mk, va, sA);
                if (FULL) {
                    sW = fma(mk, dP[o + k] - va, sW);
                    sC = fma(mk, xg[o + k], sC);
                }
            }
            accA += sA;
            accW += sW;
            accC += sC;
        }
        const int e = isx ? p.X0 + i * nx + rr : p.U0 + i * nu + rr;
        const T zz = src[e];
        out[e] = zz - alpha * accA;
        if (FULL) mx.account(alpha, pz[e], zz, accW, accC);
    }
    // x rows of the leaves: sqrtPf eta11 + eta14
    for (int it = tid; it < (p.n - p.m) * nx; it += nthr) {
        const int ll = it / nx, r = it - ll * nx, l = p.m + ll;
        const Rec lr = lrec[ll];
        const PT M = tb.SP + (size_t)lr.x * nx * nx + r;
        const int o = e11(p, l);
        T sA = T(0), sW = T(0), sC = T(0);
        for (int k = 0; k < nx; ++k) {
            const T mk = M[k * nx], va = dA[o + k];
            sA = fma(mk, va, sA);
            if (FULL) {
                sW = fma(mk, dP[o + k] - va, sW);
                sC = fma(mk, xg[o + k], sC);
            }
        }
        if (lr.z >= 0) {
            const int q = lr.z + r;
            sA += dA[q];
            if (FULL) {
                sW += dP[q] - dA[q];
                sC += xg[q];
            }
        }
        const int e = p.X0 + l * nx + r;
        const T zz = src[e];
        out[e] = zz - alpha * sA;
        if (FULL) mx.account(alpha, pz[e], zz, sW, sC);
    }
    // (y_i, tau_j, s_j) of one nonleaf node per lane: L^T, the root's s_0 relaxation and the
    // closed-form AVaR kernel projection (k_kernel_proj); the half-step values wait in `out`
    for (int i = tid; i < p.m; i += nthr) {
        const Rec fr = frec[i];
        const int c = fr.y, cs = fr.z, yo = p.Y0 + fr.x, e1o = p.E1 + fr.x;
        const T al = ((cg<T>)p.alpha_r)[i];
        const T e2A = dA[p.E2 + i];
        T e2W = T(0), e2C = T(0);
        if (FULL) {
            e2W = dP[p.E2 + i] - e2A;
            e2C = xg[p.E2 + i];
        }
        const int f2 = 2 * c;
        T y2c = src[yo + f2] - alpha * (dA[e1o + f2] - T(1) * e2A);
        if (FULL) mx.account(alpha, pz[yo + f2], src[yo + f2], (dP[e1o + f2] - dA[e1o + f2]) - T(1) * e2W, xg[e1o + f2] - T(1) * e2C);
        if (i == 0) {
            const T z0s = src[p.S0];
            out[p.S0] = (z0s - alpha * e2A) - alpha;
            if (FULL) mx.account(alpha, pz[p.S0], z0s, e2W, e2C);
        }
        T sr = T(0);
        for (int q = 0; q < c; ++q) {
            const int j = cs + q, f0 = q, f1 = c + q;
            const T b = ((cg<T>)p.cond)[j];
            const T lt0 = dA[e1o + f0] - b * e2A, lt1 = dA[e1o + f1] - T(0) * e2A;
            const T v0 = src[yo + f0] - alpha * lt0;
            const T v1 = src[yo + f1] - alpha * lt1;
            const T ltt = T(0.5) * (dA[p.E5 + j] + dA[p.E6 + j]);
            const T v2 = src[p.T0 + j] - alpha * ltt;
            const T lts = j < p.m ? dA[p.E2 + j] : T(0.5) * (dA[p.E12 + j] + dA[p.E13 + j]);
            const T v3 = src[p.S0 + j] - alpha * lts;
            if (FULL) {
                const T w0 = (dP[e1o + f0] - dA[e1o + f0]) - b * e2W, c0 = xg[e1o + f0] - b * e2C;
                const T w1 = (dP[e1o + f1] - dA[e1o + f1]) - T(0) * e2W, c1 = xg[e1o + f1] - T(0) * e2C;
                const T wt = T(0.5) * ((dP[p.E5 + j] - dA[p.E5 + j]) + (dP[p.E6 + j] - dA[p.E6 + j]));
                const T ct = T(0.5) * (xg[p.E5 + j] + xg[p.E6 + j]);
                T ws, cs2;
                if (j < p.m) {
                    ws = dP[p.E2 + j] - dA[p.E2 + j];
                    cs2 = xg[p.E2 + j];
                } else {
                    ws = T(0.5) * ((dP[p.E12 + j] - dA[p.E12 + j]) + (dP[p.E13 + j] - dA[p.E13 + j]));
                    cs2 = T(0.5) * (xg[p.E12 + j] + xg[p.E13 + j]);
                }
                mx.account(alpha, pz[yo + f0], src[yo + f0], w0, c0);
                mx.account(alpha, pz[yo + f1], src[yo + f1], w1, c1);
                mx.account(alpha, pz[p.T0 + j], src[p.T0 + j], wt, ct);
                mx.account(alpha, pz[p.S0 + j], src[p.S0 + j], ws, cs2);
            }
            out[yo + f0] = v0;
            out[yo + f1] = v1;
            out[p.T0 + j] = v2;
            out[p.S0 + j] = v3;
            sr += al * v0 - v1 + y2c - v2 - v3;
        }
        const T a = al * al + T(3);
        T sw = T(0);
        for (int q = 0; q < c; ++q) {
            const int j = cs + q, f0 = q, f1 = c + q;
            const T v0 = out[yo + f0], v1 = out[yo + f1], v2 = out[p.T0 + j], v3 = out[p.S0 + j];
            const T rk = al * v0 - v1 + y2c - v2 - v3;
            const T w = (rk - sr / (a + (T)c)) / a;
            out[yo + f0] = v0 - al * w;
            out[yo + f1] = v1 + w;
            out[p.T0 + j] = v2 + w;
            out[p.S0 + j] = v3 + w;
            sw += w;
        }
        out[yo + f2] = y2c - sw;
    }
}

// ---- projection of (x, u) of z onto the dynamics (cache.py:259-288), stage by stage
// The dynamics tables as the context holds them. double: Dev's row-major W, RG, KM, F with the
// padded row strides of raocp_dyn.hip (entry k of a row at [k]). float: the fp32 context's
// column-major M[k rows + r] tables of its per-stage dynamics (CpbArg W2 .. F2; entry k of row r
// at [k rows], so the lanes of consecutive rows read consecutive words).
template <class T>
struct DynRow {
    cg<T> ptr;
    int step;
    __device__ __forceinline__ T operator[](int k) const { return ptr[k * step]; }
};
template <class T>
__device__ __forceinline__ void dynamics_phase(const Dev& p, const CpbArg& a, const View<T>& v, gl<T>* z, int tid, int nthr) {
    constexpr bool COL = std::is_same<T, float>::value;
    const int nx = p.nx, nu = p.nu, R = nx + nu;
    const int SKP = tstride_(rup_(nx, 8)), SKF = tstride_(rup_(nx + nu, 8)), SNU = tstride_(rup_(nu, 2));
    glbrec* ninfo = (glbrec*)p.ninfo;
    glbrec* cinfo = (glbrec*)p.cinfo;
    glbi* sp = (glbi*)p.stage_ptr;
    cg<T> W = (cg<T>)(COL ? a.W2 : (const void*)p.dW), RG = (cg<T>)(COL ? a.RG2 : (const void*)p.dRG);
    cg<T> KM = (cg<T>)(COL ? a.KM2 : (const void*)p.dKM), F = (cg<T>)(COL ? a.F2 : (const void*)p.dF);
    auto row_w = [&](int kind, int rho) {
        return COL ? DynRow<T>{W + (size_t)kind * nx * R + rho, R} : DynRow<T>{W + ((size_t)kind * R + rho) * SKP, 1};
    };
    auto row_rg = [&](int cls, int tr) {
        return COL ? DynRow<T>{RG + (size_t)cls * nu * R + tr, R} : DynRow<T>{RG + ((size_t)cls * R + tr) * SNU, 1};
    };
    auto row_km = [&](int cls, int r) {
        return COL ? DynRow<T>{KM + (size_t)cls * nx * nu + r, nu} : DynRow<T>{KM + ((size_t)cls * nu + r) * SKP, 1};
    };
    auto row_f = [&](int pair, int r) {
        return COL ? DynRow<T>{F + (size_t)pair * R * nx + r, nx} : DynRow<T>{F + ((size_t)pair * nx + r) * SKF, 1};
    };
    for (int t = p.N - 1; t >= 0; --t) {
        const int b = sp[t], e = min((int)sp[t + 1], p.m);
        if (b >= e) continue;  // uniform over the workgroup
        const Rec nb = ninfo[b], ne = ninfo[e - 1];
        const int cb = nb.x, ce = ne.x + ne.y;
        // child products [h | a]_j = sign [B'; A'] q_j (a leaf child: q_j = -x_j)
        for (int it = tid; it < (ce - cb) * R; it += nthr) {
            const int jj = it / R, rho = it - jj * R, j = cb + jj;
            const Rec cj = cinfo[j];
            const DynRow<T> w = row_w(cj.x, rho);
            cg<T> qv = j < p.m ? (cg<T>)v.q + (size_t)j * nx : (cg<T>)z + p.X0 + (size_t)j * nx;
            T acc = T(0);
            for (int k = 0; k < nx; ++k) acc = fma(w[k], qv[k], acc);
            v.pb[(size_t)j * R + rho] = j < p.m ? acc : -acc;
        }
        __syncthreads();
        // d = Rinv v, q = (-x + a) + G v with v = u - sum_j h_j
        for (int it = tid; it < (e - b) * R; it += nthr) {
            const int ii = it / R, tr = it - ii * R, i = b + ii;
            const Rec ni = ninfo[i];
            const DynRow<T> rg = row_rg(ni.z, tr);
            cg<T> u = (cg<T>)z + p.U0 + (size_t)i * nu;
            T s = T(0);
            for (int k = 0; k < nu; ++k) {
                T vk = u[k];
                for (int q = 0; q < ni.y; ++q) vk -= v.pb[(size_t)(ni.x + q) * R + k];
                s = fma(rg[k], vk, s);
            }
            if (tr < nu) {
                v.dd[(size_t)i * nu + tr] = s;
            } else {
                const int r = tr - nu;
                T a = T(0);
                for (int q = 0; q < ni.y; ++q) a += v.pb[(size_t)(ni.x + q) * R + nu + r];
                v.q[(size_t)i * nx + r] = (-z[p.X0 + (size_t)i * nx + r] + a) + s;
            }
        }
        __syncthreads();
    }
    if (tid < nx) z[p.X0 + tid] = v.x0[tid];  // x_0 = x0bar (cache.py:282)
    __syncthreads();
    for (int t = 0; t < p.N; ++t) {
        const int b = sp[t], e = min((int)sp[t + 1], p.m);
        if (b >= e) continue;
        const Rec nb = ninfo[b], ne = ninfo[e - 1];
        const int cb = nb.x, ce = ne.x + ne.y;
        const int nU = (e - b) * nu, nX = (ce - cb) * nx;
        for (int it = tid; it < nU + nX; it += nthr) {
            if (it < nU) {
                const int ii = it / nu, r = it - ii * nu, i = b + ii;
                const Rec ni = ninfo[i];
                const DynRow<T> km = row_km(ni.z, r);
                cg<T> x = (cg<T>)z + p.X0 + (size_t)i * nx;
                T s = T(0);
                for (int k = 0; k < nx; ++k) s = fma(km[k], x[k], s);
                z[p.U0 + (size_t)i * nu + r] = s + v.dd[(size_t)i * nu + r];
            } else {
                const int wi = it - nU, jj = wi / nx, r = wi - jj * nx, j = cb + jj;
                const Rec cj = cinfo[j];
                const DynRow<T> f = row_f(cj.y, r);
                cg<T> x = (cg<T>)z + p.X0 + (size_t)cj.z * nx;
                cg<T> dv = (cg<T>)v.dd + (size_t)cj.z * nu;
                T s = T(0);
                for (int k = 0; k < nx; ++k) s = fma(f[k], x[k], s);
                for (int k = 0; k < nu; ++k) s = fma(f[nx + k], dv[k], s);
                z[p.X0 + (size_t)j * nx + r] = s;
            }
        }
        __syncthreads();
    }
}

// ---- the dual rows. PASS 1: v = (d + alpha L(2 z+ - p)) / alpha (+-1/2) -> tv, L(z+ - p) -> xi2.
// PASS 2: eta+ = alpha (v - Pi(v)) -> eo, xi2 = (d - eta+) / alpha + L(z+ - p), |xi2|, |delta2|.
// Rows: per child j >= 1 eta3 (nx), eta4 (nu), eta5, eta6 (one SOC); per nonleaf i eta1
// (2c + 1), eta2, eta7 (nx + nu, a box when the node has one); per leaf eta11 (nx), eta12,
// eta13 (one SOC), eta14 (nx, a box when the leaf has one).
template <class T, int PASS, class PT>
__device__ __forceinline__ void dual_phase(const Dev& p, const Tabs<PT>& tb, const View<T>& v, T alpha, Maxima<T>& mx,
                                           bool& nan, int tid, int nthr) {
    const int nx = p.nx, nu = p.nu;
    cg<T> pz = v.pz, zp = v.zp, d = v.d;
    glbrec* frec = (glbrec*)p.frec;
    glbrec* crec = (glbrec*)p.crec;
    glbrec* lrec = (glbrec*)p.lrec;
    auto put = [&](int e, T av, T bb, T shift) {
        const T vv = (d[e] + alpha * av) / alpha + shift;
        v.tv[e] = vv;
        v.xi2[e] = bb;
    };
    auto finish = [&](int e, T vv, T pv) {
        const T dv = d[e], bb = v.xi2[e];
        const T ep = alpha * (vv - pv);
        v.eo[e] = ep;
        const T x2 = (dv - ep) / alpha + bb;
        v.xi2[e] = x2;
        mx.m2 = nmx<T>(mx.m2, fabs(x2));
        mx.m5 = nmx<T>(mx.m5, fabs(ep - dv));
    };
    const int GC = nx + nu + 2;
    for (int it = tid; it < (p.n - 1) * GC; it += nthr) {
        const int jj = it / GC, r = it - jj * GC, j = 1 + jj;
        const int e = r < nx ? e3(p, j) + r : (r < nx + nu ? e4(p, j) + r - nx : (r == nx + nu ? p.E5 : p.E6) + j);
        if (PASS == 1) {
            const Rec cr = crec[j];
            T av, bb, shift = T(0);
            if (r < nx + nu) {
                const bool isx = r < nx;
                const int rr = isx ? r : r - nx, len = isx ? nx : nu;
                const PT M = isx ? tb.SQ + (size_t)cr.y * nx * nx + rr : tb.SR + (size_t)cr.z * nu * nu + rr;
                const int o = isx ? p.X0 + cr.x * nx : p.U0 + cr.x * nu;
                T sa = T(0), sb = T(0);
                for (int k = 0; k < len; ++k) {
                    const T mk = M[k * len], zk = zp[o + k], pk = pz[o + k];
                    sa = fma(mk, T(2) * zk - pk, sa);
                    sb = fma(mk, zk - pk, sb);
                }
                av = sa;
                bb = sb;
            } else {
                const T zt = zp[p.T0 + j], pt = pz[p.T0 + j];
                av = T(0.5) * (T(2) * zt - pt);
                bb = T(0.5) * (zt - pt);
                shift = r == nx + nu ? T(-0.5) : T(0.5);
            }
            put(e, av, bb, shift);
        } else {
            T ss = T(0);
            const int o3 = e3(p, j), o4 = e4(p, j);
            for (int q = 0; q < nx; ++q) ss += v.tv[o3 + q] * v.tv[o3 + q];
            for (int q = 0; q < nu; ++q) ss += v.tv[o4 + q] * v.tv[o4 + q];
            ss += v.tv[p.E5 + j] * v.tv[p.E5 + j];
            const T vv = v.tv[e];
            finish(e, vv, soc_apply(vv, r == GC - 1, sqrt(ss), v.tv[p.E6 + j]));
        }
    }
    const int GP = 2 * p.cmax + 2 + nx + nu;
    for (int it = tid; it < p.m * GP; it += nthr) {
        const int i = it / GP, r = it - i * GP;
        const Rec fr = frec[i];
        const int c = fr.y, yo = p.Y0 + fr.x, cs = fr.z;
        if (r < 2 * c + 1) {
            const int e = p.E1 + fr.x + r;
            if (PASS == 1) {
                const T zy = zp[yo + r], py = pz[yo + r];
                put(e, T(2) * zy - py, zy - py, T(0));
            } else {
                const T vv = v.tv[e];
                finish(e, vv, r < 2 * c ? fmax(vv, T(0)) : vv);
            }
        } else if (r == 2 * p.cmax + 1) {
            const int e = p.E2 + i;
            if (PASS == 1) {
                T bya = T(0), byb = T(0);
                for (int k = 0; k < c; ++k) {
                    const T cp = ((cg<T>)p.cond)[cs + k];
                    bya = fma(cp, T(2) * zp[yo + k] - pz[yo + k], bya);
                    byb = fma(cp, zp[yo + k] - pz[yo + k], byb);
                }
                bya += T(2) * zp[yo + 2 * c] - pz[yo + 2 * c];
                byb += zp[yo + 2 * c] - pz[yo + 2 * c];
                const T zs = zp[p.S0 + i], ps = pz[p.S0 + i];
                put(e, (T(2) * zs - ps) - bya, (zs - ps) - byb, T(0));
            } else {
                const T vv = v.tv[e];
                finish(e, vv, fmax(vv, T(0)));
            }
        } else if (r >= 2 * p.cmax + 2 && fr.w >= 0) {
            const int rr = r - (2 * p.cmax + 2);
            const int e = fr.w + rr;
            if (PASS == 1) {
                const int o = rr < nx ? p.X0 + i * nx + rr : p.U0 + i * nu + rr - nx;
                const T zv = zp[o], pv = pz[o];
                put(e, T(2) * zv - pv, zv - pv, T(0));
            } else {
                const int bi = ((glbi*)p.iBnl)[i];
                const T vv = v.tv[e];
                finish(e, vv, box_apply(vv, tb.BLn[(size_t)bi * (nx + nu) + rr], tb.BHn[(size_t)bi * (nx + nu) + rr], nan));
            }
        }
    }
    const int GL = 2 * nx + 2;
    for (int it = tid; it < (p.n - p.m) * GL; it += nthr) {
        const int ll = it / GL, r = it - ll * GL, l = p.m + ll;
        const Rec lr = lrec[ll];
        if (r < nx + 2) {
            const int e = r < nx ? e11(p, l) + r : (r == nx ? p.E12 : p.E13) + l;
            if (PASS == 1) {
                T av, bb, shift = T(0);
                if (r < nx) {
                    const PT M = tb.SP + (size_t)lr.x * nx * nx + r;
                    const int o = p.X0 + l * nx;
                    T sa = T(0), sb = T(0);
                    for (int k = 0; k < nx; ++k) {
                        const T mk = M[k * nx], zk = zp[o + k], pk = pz[o + k];
                        sa = fma(mk, T(2) * zk - pk, sa);
                        sb = fma(mk, zk - pk, sb);
                    }
                    av = sa;
                    bb = sb;
                } else {
                    const T zs = zp[p.S0 + l], ps = pz[p.S0 + l];
                    av = T(0.5) * (T(2) * zs - ps);
                    bb = T(0.5) * (zs - ps);
                    shift = r == nx ? T(-0.5) : T(0.5);
                }
                put(e, av, bb, shift);
            } else {
                T ss = T(0);
                const int o11 = e11(p, l);
                for (int q = 0; q < nx; ++q) ss += v.tv[o11 + q] * v.tv[o11 + q];
                ss += v.tv[p.E12 + l] * v.tv[p.E12 + l];
                const T vv = v.tv[e];
                finish(e, vv, soc_apply(vv, r == nx + 1, sqrt(ss), v.tv[p.E13 + l]));
            }
        } else if (lr.z >= 0) {
            const int rr = r - nx - 2;
            const int e = lr.z + rr;
            if (PASS == 1) {
                const T zv = zp[p.X0 + l * nx + rr], pv = pz[p.X0 + l * nx + rr];
                put(e, T(2) * zv - pv, zv - pv, T(0));
            } else {
                const T vv = v.tv[e];
                finish(e, vv, box_apply(vv, tb.BLl[(size_t)lr.y * nx + rr], tb.BHl[(size_t)lr.y * nx + rr], nan));
            }
        }
    }
}

template <class T>
__device__ __forceinline__ T wave_max(T v) {
    for (int off = 32; off > 0; off >>= 1) v = nmx<T>(v, __shfl_xor(v, off, 64));
    return v;
}

template <class T>
__device__ __forceinline__ View<T> view_of(T* slab, const CpbSlab& L, int k) {
    View<T> v;
    v.pz = (gl<T>*)(slab + L.z[k % 3]);
    v.zp = (gl<T>*)(slab + L.z[(k + 1) % 3]);
    v.out = (gl<T>*)(slab + L.z[(k + 2) % 3]);
    v.d = (gl<T>*)(slab + L.e[k % 2]);
    v.eo = (gl<T>*)(slab + L.e[(k + 1) % 2]);
    v.xi2 = (gl<T>*)(slab + L.xi2);
    v.tv = (gl<T>*)(slab + L.tv);
    v.q = (gl<T>*)(slab + L.q);
    v.dd = (gl<T>*)(slab + L.dd);
    v.pb = (gl<T>*)(slab + L.pb);
    v.x0 = (cg<T>)(slab + L.x0);
    return v;
}

// The residual maxima are taken in T; the history row is their widening to double (exact) and
// the stopping test compares in double, as cp_check_wave does on an fp32 context.
template <class T, class PT>
__device__ __forceinline__ void cpb_body(const Dev& p, const CpbArg& a, const Tabs<PT>& tb, int b) {
    __shared__ T s_red[6][kCpbBlock / 64];
    __shared__ int s_ctl[2];  // {done, k} of the instance, as thread 0 left them
    const int tid = threadIdx.x, nthr = blockDim.x;
    Ctl* ctl = a.ctl + b;
    T* slab = (T*)a.slab + (size_t)b * a.lay.stride;
    double* hist = a.hist + (size_t)b * a.hist_rows * 6;
    const T alpha = (T)ctl->alpha;
    int k = ctl->k;
    if (!ctl->pad) {
        // the solve's first half step Z[1] = prox-part(Z[0] - alpha L^T E[0])
        const View<T> v = view_of(slab, a.lay, 0);
        Maxima<T> none;
        primal_phase<T, false>(p, tb, v, v.zp, alpha, none, tid, nthr);
        __syncthreads();
        if (tid == 0) ctl->pad = 1;
    }
    for (int it = 0; it < a.chunk; ++it) {
        const View<T> v = view_of(slab, a.lay, k);
        Maxima<T> mx;
        bool nan = false;
        dynamics_phase<T>(p, a, v, v.zp, tid, nthr);
        dual_phase<T, 1>(p, tb, v, alpha, mx, nan, tid, nthr);
        __syncthreads();
        dual_phase<T, 2>(p, tb, v, alpha, mx, nan, tid, nthr);
        __syncthreads();
        primal_phase<T, true>(p, tb, v, v.out, alpha, mx, tid, nthr);
        // the six maxima of the instance, its history row and the stopping test (cp_check_wave)
        const T mm[6] = {wave_max(mx.m0), wave_max(mx.m1), wave_max(mx.m2),
                              wave_max(mx.m3), wave_max(mx.m4), wave_max(mx.m5)};
        if ((tid & 63) == 0) _Pragma("unroll") for (int q = 0; q < 6; ++q) s_red[q][tid >> 6] = mm[q];
        const int any_nan = __syncthreads_or(nan ? 1 : 0);
        if (tid == 0) {
            T m[6];
            _Pragma("unroll") for (int q = 0; q < 6; ++q) {
                T r = s_red[q][0];
                for (int w = 1; w < (nthr >> 6); ++w) r = nmx<T>(r, s_red[q][w]);
                m[q] = r;
                hist[(size_t)k * 6 + q] = (double)r;
            }
            const double err = (double)nmx<T>(nmx<T>(m[0], m[1]), m[2]);
            int done = 0;
            if (any_nan) ctl->flags |= 1;
            if (k >= ctl->max_iters || err <= ctl->tol || any_nan) {
                ctl->done = 1;
                ctl->final_k = k;
                a.done[b] = 1;
                done = 1;
            } else {
                ctl->k = k + 1;
            }
            s_ctl[0] = done;
            s_ctl[1] = done ? k : k + 1;
        }
        __syncthreads();
        const int done = s_ctl[0];
        k = s_ctl[1];
        if (done) {
            if (tid < p.nu) a.u0[(size_t)b * p.nu + tid] = (double)v.zp[p.U0 + tid];
            break;
        }
    }
}

template <class T, bool LT>
__global__ void __launch_bounds__(kCpbBlock) k_cpb(Dev p, CpbArg a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_[];
    const int b = blockIdx.x;
    if (b >= a.B || a.ctl[b].done) return;  // a finished instance leaves at kernel entry
    const int nx = p.nx, nu = p.nu;
    const int nQ = p.nSQ * nx * nx, nR = p.nSR * nu * nu, nP = p.nSP * nx * nx, nBn = p.nBnl * (nx + nu), nBl = p.nBl * nx;
    if constexpr (LT) {
        __attribute__((address_space(3))) T* s = (__attribute__((address_space(3))) T*)smem_;
        const cg<T> src[7] = {(cg<T>)p.SQ, (cg<T>)p.SR, (cg<T>)p.SP, (cg<T>)p.blo_nl, (cg<T>)p.bhi_nl, (cg<T>)p.blo_l, (cg<T>)p.bhi_l};
        const int cnt[7] = {nQ, nR, nP, nBn, nBn, nBl, nBl};
        int off[8];
        off[0] = 0;
        _Pragma("unroll") for (int t = 0; t < 7; ++t) off[t + 1] = off[t] + cnt[t];
        _Pragma("unroll") for (int t = 0; t < 7; ++t)
            for (int e = threadIdx.x; e < cnt[t]; e += blockDim.x) s[off[t] + e] = src[t][e];
        __syncthreads();
        const Tabs<cl<T>> tb{s + off[0], s + off[1], s + off[2], s + off[3], s + off[4], s + off[5], s + off[6]};
        cpb_body<T>(p, a, tb, b);
    } else {
        const Tabs<cg<T>> tb{(cg<T>)p.SQ, (cg<T>)p.SR, (cg<T>)p.SP, (cg<T>)p.blo_nl, (cg<T>)p.bhi_nl, (cg<T>)p.blo_l, (cg<T>)p.bhi_l};
        cpb_body<T>(p, a, tb, b);
    }
}

// ---- k_cpa: k_cpb's iteration with Anderson acceleration, fp64 only.
// With v = (z, eta), g_k = T(v_k) the iteration above and r_k = g_k - v_k, after the phases of
// iteration k:
//   A. one pass over the P + D entries: r_k, the new difference column (g_k - g_prev,
//      r_k - r_prev) into the ring slot `head` when a previous pair is held, the pair itself, and
//      per lane the partial sums of |r_k|^2, of b = dR' r_k and of the new row of G = dR' dR
//      (double; a wave shuffle tree, then the waves in index order by thread 0)
//   B. thread 0: the history row and the stopping test as in k_cpb; a pending trial is accepted
//      when |r_k|_2 <= safeguard |r_saved|_2, else rejected (history cleared, g_saved comes back;
//      a rejected trial does not stop on the tolerance); otherwise the push is committed and,
//      when (k + 1) % every == 0, gamma = (G + reg (tr G / j) I)^-1 b (aa_solve); the log record
//   C. a proposal: g_k is saved and v^ = g_k - dG gamma takes its place in Z[(k + 1) % 3],
//      E[(k + 1) % 2]; a rejection: the saved g_k goes there. Either way the half step
//      Z[(k + 2) % 3] is computed again from that pair, as the solve's first half step is.
// The pass writes only the acceleration slab, so what it leaves after the iteration that ends
// the solve, or before a rejection clears the history, is never read. All state between two
// iterations is in the slabs and Ctl: a launch may end between a proposal and its trial.
template <class T, class PT>
__device__ __forceinline__ void cpa_body(const Dev& p, const CpbArg& a, const CpaArg& aa, const Tabs<PT>& tb, int b) {
    static_assert(std::is_same<T, double>::value, "k_cpa is fp64 only");
    constexpr int M8 = kAaMaxM, NW = kCpbBlock / 64, ND = 2 * M8 + 1;
    __shared__ T s_red[6][NW];
    __shared__ double s_dot[ND][NW];
    __shared__ double s_gam[M8], s_b[M8], s_G[M8 * M8], s_L[M8 * M8];
    __shared__ int s_slot[M8];
    __shared__ int s_st[4];   // head, count, have, pending: as thread 0 left them
    __shared__ int s_ctl[3];  // {done, k, action} of the instance; action 1 proposal, 2 restore
    const int tid = threadIdx.x, nthr = blockDim.x;
    Ctl* ctl = a.ctl + b;
    T* slab = (T*)a.slab + (size_t)b * a.lay.stride;
    double* hist = a.hist + (size_t)b * a.hist_rows * 6;
    double* log = aa.log + (size_t)b * a.hist_rows * kAaRec;
    const CpaSlab& A = aa.lay;
    double* as = aa.slab + (size_t)b * A.stride;
    gl<double>* dG = (gl<double>*)(as + A.dg);
    gl<double>* dR = (gl<double>*)(as + A.dr);
    gl<double>* pg = (gl<double>*)(as + A.pg);
    gl<double>* pr = (gl<double>*)(as + A.pr);
    gl<double>* sg = (gl<double>*)(as + A.sg);
    double* Gm = as + A.G;
    CpaState* st = (CpaState*)(as + A.state);
    const int m = A.m, P = p.P, NE = p.P + p.D;
    const long vec = A.vec;
    const T alpha = (T)ctl->alpha;
    int k = ctl->k;
    if (tid == 0) {
        s_st[0] = st->head;
        s_st[1] = st->count;
        s_st[2] = st->have;
        s_st[3] = st->pending;
    }
    if (!ctl->pad) {
        const View<T> v = view_of(slab, a.lay, 0);
        Maxima<T> none;
        primal_phase<T, false>(p, tb, v, v.zp, alpha, none, tid, nthr);
        __syncthreads();
        if (tid == 0) ctl->pad = 1;
    }
    __syncthreads();
    for (int it = 0; it < a.chunk; ++it) {
        const View<T> v = view_of(slab, a.lay, k);
        Maxima<T> mx;
        bool nan = false;
        dynamics_phase<T>(p, a, v, v.zp, tid, nthr);
        dual_phase<T, 1>(p, tb, v, alpha, mx, nan, tid, nthr);
        __syncthreads();
        dual_phase<T, 2>(p, tb, v, alpha, mx, nan, tid, nthr);
        __syncthreads();
        primal_phase<T, true>(p, tb, v, v.out, alpha, mx, tid, nthr);
        // A. the acceleration pass
        const int head = s_st[0], count = s_st[1], have = s_st[2], pending = s_st[3];
        const int ncol = have ? min(count + 1, m) : count;  // columns once the push is committed
        double acc[ND];
        _Pragma("unroll") for (int q = 0; q < ND; ++q) acc[q] = 0.0;
        for (int e = tid; e < NE; e += nthr) {
            const double gv = e < P ? v.zp[e] : v.eo[e - P];
            const double vv = e < P ? v.pz[e] : v.d[e - P];
            const double r = gv - vv;
            double drn = 0.0;
            if (have) {
                drn = r - pr[e];
                dR[(size_t)head * vec + e] = drn;
                dG[(size_t)head * vec + e] = gv - pg[e];
            }
            pg[e] = gv;
            pr[e] = r;
            acc[2 * M8] = fma(r, r, acc[2 * M8]);
            _Pragma("unroll") for (int s = 0; s < M8; ++s)
                if (s < ncol) {
                    const double c = (have && s == head) ? drn : dR[(size_t)s * vec + e];
                    acc[M8 + s] = fma(c, r, acc[M8 + s]);
                    acc[s] = fma(c, drn, acc[s]);
                }
        }
        _Pragma("unroll") for (int q = 0; q < ND; ++q) {
            double s = acc[q];
            for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
            acc[q] = s;
        }
        const T mm[6] = {wave_max(mx.m0), wave_max(mx.m1), wave_max(mx.m2),
                              wave_max(mx.m3), wave_max(mx.m4), wave_max(mx.m5)};
        if ((tid & 63) == 0) {
            _Pragma("unroll") for (int q = 0; q < 6; ++q) s_red[q][tid >> 6] = mm[q];
            _Pragma("unroll") for (int q = 0; q < ND; ++q) s_dot[q][tid >> 6] = acc[q];
        }
        const int any_nan = __syncthreads_or(nan ? 1 : 0);
        // B. the history row, the stopping test and the acceleration's decision
        if (tid == 0) {
            T mr[6];
            _Pragma("unroll") for (int q = 0; q < 6; ++q) {
                T r = s_red[q][0];
                for (int w = 1; w < (nthr >> 6); ++w) r = nmx<T>(r, s_red[q][w]);
                mr[q] = r;
                hist[(size_t)k * 6 + q] = (double)r;
            }
            // the waves' partial sums in index order
            auto dsum = [&](int q) {
                double s = s_dot[q][0];
                for (int w = 1; w < (nthr >> 6); ++w) s += s_dot[q][w];
                return s;
            };
            const double err = (double)nmx<T>(nmx<T>(mr[0], mr[1]), mr[2]);
            const double rn = sqrt(dsum(2 * M8));
            for (int i = 0; i < M8; ++i) s_gam[i] = 0.0;
            int code = 0, prop = 0, action = 0, jlog = 0;
            int nh = head, nc = count, nhave = have, npend = 0;
            bool rejected = false;
            if (pending) {
                const bool accept = rn <= aa.safeguard * st->rnorm;
                code = accept ? 2 : 3;
                rejected = !accept;
            }
            if (any_nan) ctl->flags |= 1;
            const bool stop = k >= ctl->max_iters || any_nan || (!rejected && err <= ctl->tol);
            if (stop) {
                ctl->done = 1;
                ctl->final_k = k;
                a.done[b] = 1;
            } else if (rejected) {
                nh = nc = nhave = 0;
                action = 2;
            } else {
                if (have) {  // the push is committed: the new row and column of G
                    for (int s = 0; s < ncol; ++s) Gm[head * M8 + s] = Gm[s * M8 + head] = dsum(s);
                    nh = (head + 1) % m;
                    nc = ncol;
                }
                nhave = 1;
                jlog = nc;
                if (nc >= 1 && (k + 1) % aa.every == 0) {
                    // the columns oldest first
                    for (int i = 0; i < nc; ++i) {
                        const int si = (nh - nc + i + m) % m;
                        s_slot[i] = si;
                        s_b[i] = dsum(M8 + si);
                        for (int j = 0; j <= i; ++j) s_G[i * M8 + j] = Gm[si * M8 + s_slot[j]];
                    }
                    if (aa_solve(nc, (lds<double>*)s_G, (lds<double>*)s_b, aa.reg, (lds<double>*)s_gam, (lds<double>*)s_L)) {
                        action = 1;
                        npend = 1;
                        st->rnorm = rn;
                        prop = 1;
                        if (code == 0) code = 1;
                    } else {
                        for (int i = 0; i < M8; ++i) s_gam[i] = 0.0;
                        nh = nc = nhave = 0;
                        prop = 2;
                        if (code == 0) code = 4;
                    }
                }
            }
            if (!stop) ctl->k = k + 1;
            double* rec = log + (size_t)k * kAaRec;
            rec[0] = (double)code;
            rec[1] = (double)jlog;
            rec[2] = (double)prop;
            rec[3] = rn;
            for (int i = 0; i < M8; ++i) rec[4 + i] = s_gam[i];
            st->head = s_st[0] = nh;
            st->count = s_st[1] = nc;
            st->have = s_st[2] = nhave;
            st->pending = s_st[3] = npend;
            s_ctl[0] = stop ? 1 : 0;
            s_ctl[1] = stop ? k : k + 1;
            s_ctl[2] = action;
        }
        __syncthreads();
        const int done = s_ctl[0], action = s_ctl[2];
        k = s_ctl[1];
        if (done) {
            if (tid < p.nu) a.u0[(size_t)b * p.nu + tid] = (double)v.zp[p.U0 + tid];
            break;
        }
        // C. the next iterate is not g_k: put it in place and redo the half step from it
        if (action) {
            const int nc = s_st[1];
            for (int e = tid; e < NE; e += nthr) {
                gl<T>* dst = e < P ? v.zp + e : v.eo + (e - P);
                if (action == 1) {
                    const double gv = *dst;
                    sg[e] = gv;
                    double s = gv;
                    for (int i = 0; i < nc; ++i) s = fma(-s_gam[i], dG[(size_t)s_slot[i] * vec + e], s);
                    *dst = s;
                } else {
                    *dst = sg[e];
                }
            }
            __syncthreads();
            const View<T> vn = view_of(slab, a.lay, k);
            Maxima<T> none;
            primal_phase<T, false>(p, tb, vn, vn.zp, alpha, none, tid, nthr);
            __syncthreads();
        }
    }
}

template <class T, bool LT>
__global__ void __launch_bounds__(kCpbBlock) k_cpa(Dev p, CpbArg a, CpaArg aa) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_[];
    const int b = blockIdx.x;
    if (b >= a.B || a.ctl[b].done) return;  // a finished instance leaves at kernel entry
    const int nx = p.nx, nu = p.nu;
    const int nQ = p.nSQ * nx * nx, nR = p.nSR * nu * nu, nP = p.nSP * nx * nx, nBn = p.nBnl * (nx + nu), nBl = p.nBl * nx;
    if constexpr (LT) {
        __attribute__((address_space(3))) T* s = (__attribute__((address_space(3))) T*)smem_;
        const cg<T> src[7] = {(cg<T>)p.SQ, (cg<T>)p.SR, (cg<T>)p.SP, (cg<T>)p.blo_nl, (cg<T>)p.bhi_nl, (cg<T>)p.blo_l, (cg<T>)p.bhi_l};
        const int cnt[7] = {nQ, nR, nP, nBn, nBn, nBl, nBl};
        int off[8];
        off[0] = 0;
        _Pragma("unroll") for (int t = 0; t < 7; ++t) off[t + 1] = off[t] + cnt[t];
        _Pragma("unroll") for (int t = 0; t < 7; ++t)
            for (int e = threadIdx.x; e < cnt[t]; e += blockDim.x) s[off[t] + e] = src[t][e];
        __syncthreads();
        const Tabs<cl<T>> tb{s + off[0], s + off[1], s + off[2], s + off[3], s + off[4], s + off[5], s + off[6]};
        cpa_body<T>(p, a, aa, tb, b);
    } else {
        const Tabs<cg<T>> tb{(cg<T>)p.SQ, (cg<T>)p.SR, (cg<T>)p.SP, (cg<T>)p.blo_nl, (cg<T>)p.bhi_nl, (cg<T>)p.blo_l, (cg<T>)p.bhi_l};
        cpa_body<T>(p, a, aa, tb, b);
    }
}

// ---- k_mpc_step: the end of step t of a closed-loop simulation and the start of step t + 1,
// one workgroup per instance, launched after every instance of the batch is done with step t.
//   1. x = the slab's x0, u = the root's input of the final primal Z[(final_k + 1) % 3]; with
//      i = ch_start[0] + scen[b][t]: x+ = A_i x + B_i u (one lane per row, k ascending, fma) and
//      l = |SQ_i x|^2 + |SR_i u|^2 (one lane per row of SQ_i / SR_i, lane 0 adds the squares in
//      row order); X[b][t + 1], U[b][t], cost[b][t], status, iters and the xi maxima of the last
//      history row are recorded
//   2. unless this was the last step: the final iterate moves to Z[0] / E[0] (warm; 16-B
//      copies, skipped when it is there already), the rest of the slab is cleared as the
//      host's memset of a fresh batch leaves it (16-B stores), x+ goes to node 0's state of
//      Z[0] and to the slab's x0, and the instance's Ctl and done word are reset.
// An instance whose solve raised the NaN flag is frozen: its slab, Ctl and done word stay, this
// step and every later one record status 2 (later ones: 0 iterations) and NaN for x+, u, l.
// The plant step and the stage cost are computed in T; the records X, U, cost and err are double
// for either T (widened at the store), status and iters int.
//
// k_mpc_step_aa (AA, fp64 only) is the same step after a solve of k_cpa, and in addition
//   0. counts: the lanes stride over the records 0 .. final_k of the instance's log, each adds what
//      aa_count (raocp_aa_ops.h) says to its four counters; a wave shuffle tree, then the four
//      waves in index order from LDS, stored to counts[b][t]. An instance frozen at an earlier
//      step stores zeros, the step that freezes it the counts of the solve that froze it.
//   3. unless this was the last step: the instance's CpaState (pending flag and stored |r|_2
//      included) and its G block are cleared with 16-B stores, so the next step's first k_cpa
//      iteration sees what the memset of a fresh accelerated batch leaves: an empty history,
//      whatever `warm` is. The last step leaves state and log in place for raocp_cp_batch_aa_log.
// The iterate that is applied and carried over is Z[(final_k + 1) % 3] / E[(final_k + 1) % 2] as
// after k_cpb: cpa_body decides `stop` before it considers a proposal, so the iteration that ends a
// solve (through max_iters as through tol or a NaN) never writes one over g_k, and that slot holds
// the last T(.) computed, which is also what it stores to u0 and what raocp_cp_batch_get reads.
// (The arguments by value, as a kernel takes them: k_mpc_step<double> / <float> then keep the
// resource lines they had before the body was shared, 40 / 24 VGPRs, 80 SGPRs, no scratch.)
template <class T, bool AA>
__device__ __forceinline__ void mpc_step_body(const Dev p, const CpbArg a, const MpcArg m, const CpaArg* aa, int* counts) {
    // 16 bytes of the slab: 2 doubles or 4 floats
    constexpr int VN = 16 / (int)sizeof(T);
    typedef T vt __attribute__((ext_vector_type(VN)));
    typedef __attribute__((address_space(1))) vt glbvt;
    __shared__ T s_x[kCpbMaxNx], s_u[kCpbMaxNu], s_xp[kCpbMaxNx], s_sq[kCpbMaxNx + kCpbMaxNu];
    const int b = blockIdx.x;
    if (b >= a.B) return;
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int nx = p.nx, nu = p.nu, NT = m.T, t = m.t;
    Ctl* ctl = a.ctl + b;
    T* slab = (T*)a.slab + (size_t)b * a.lay.stride;
    gl<double>* Xo = (gl<double>*)(m.X + ((size_t)b * (NT + 1) + t) * nx);
    gl<double>* Uo = (gl<double>*)(m.U + ((size_t)b * NT + t) * nu);
    const size_t bt = (size_t)b * NT + t;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    // uniform over the workgroup: nobody writes these words before the barrier below
    const int fk = ctl->final_k, flags = ctl->flags, max_iters = ctl->max_iters;
    const int frz = m.frz[b];
    cg<T> x = (cg<T>)(slab + a.lay.x0);
    if (t == 0 && tid < nx) Xo[tid] = (double)x[tid];
    if constexpr (AA) {
        __shared__ int s_cnt[kAaCounts][kCpbBlock / 64];
        const int rows = frz >= 0 ? 0 : fk + 1;
        cg<double> lg = (cg<double>)(aa->log + (size_t)b * a.hist_rows * kAaRec);
        int cnt[kAaCounts] = {0, 0, 0, 0};
        for (int r = tid; r < rows; r += nthr) aa_count((int)lg[(size_t)r * kAaRec], (int)lg[(size_t)r * kAaRec + 2], cnt);
        _Pragma("unroll") for (int q = 0; q < kAaCounts; ++q) {
            int c = cnt[q];
            for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
            if ((tid & 63) == 0) s_cnt[q][tid >> 6] = c;
        }
        __syncthreads();
        if (tid < kAaCounts) {
            int c = s_cnt[tid][0];
            for (int w = 1; w < (nthr >> 6); ++w) c += s_cnt[tid][w];
            ((gl<int>*)counts)[bt * kAaCounts + tid] = c;
        }
    }
    if (frz >= 0 || (flags & 1)) {
        if (tid < nx) Xo[nx + tid] = qnan;
        if (tid < nu) Uo[tid] = qnan;
        if (tid < 3) m.err[bt * 3 + tid] = frz >= 0 ? qnan : a.hist[((size_t)b * a.hist_rows + fk) * 6 + tid];
        if (tid == 0) {
            m.cost[bt] = qnan;
            m.status[bt] = 2;
            m.iters[bt] = frz >= 0 ? 0 : fk + 1;
        }
        __syncthreads();  // every lane has read frz[b]
        if (tid == 0 && frz < 0) m.frz[b] = t;
        return;
    }
    const int zs = (fk + 1) % 3, es = (fk + 1) % 2;
    cg<T> zf = (cg<T>)(slab + a.lay.z[zs]);
    if (tid < nx) s_x[tid] = x[tid];
    if (tid < nu) s_u[tid] = zf[p.U0 + tid];
    __syncthreads();
    const int j = m.scen[bt];
    const int i = ((glbi*)p.ch_start)[0] + j;
    const Rec cr = ((glbrec*)p.crec)[i];
    if (tid < nx) {
        cg<T> Ar = (cg<T>)m.ab + ((size_t)j * (nx + nu) + tid) * nx;
        cg<T> Br = (cg<T>)m.ab + ((size_t)j * (nx + nu) + nx) * nx + (size_t)tid * nu;
        T s = T(0);
        for (int k = 0; k < nx; ++k) s = fma(Ar[k], s_x[k], s);
        for (int k = 0; k < nu; ++k) s = fma(Br[k], s_u[k], s);
        s_xp[tid] = s;
        Xo[nx + tid] = (double)s;
    } else if (tid >= 64 && tid < 64 + nx + nu) {
        // the column-major L weights: M[k * rows + r] = M_rk
        const int r = tid - 64;
        const bool isx = r < nx;
        const int rr = isx ? r : r - nx, len = isx ? nx : nu;
        cg<T> M = isx ? (cg<T>)p.SQ + (size_t)cr.y * nx * nx + rr : (cg<T>)p.SR + (size_t)cr.z * nu * nu + rr;
        const T* v = isx ? s_x : s_u;
        T s = T(0);
        for (int k = 0; k < len; ++k) s = fma(M[k * len], v[k], s);
        s_sq[r] = s * s;
    }
    if (tid < nu) Uo[tid] = (double)s_u[tid];
    if (tid < 3) m.err[bt * 3 + tid] = a.hist[((size_t)b * a.hist_rows + fk) * 6 + tid];
    __syncthreads();
    if (tid == 0) {
        T l = T(0);
        for (int r = 0; r < nx + nu; ++r) l += s_sq[r];
        m.cost[bt] = (double)l;
        m.status[bt] = fk < max_iters ? 0 : 1;
        m.iters[bt] = fk + 1;
    }
    if (m.last) return;
    // every array of the slab starts on a 16-B boundary and its length in the layout is a whole
    // number of 16-B vectors, the stride a multiple of 256 B (cpb_layout_dims: Z[0] at the slab's
    // start, then Z[1], Z[2], E[0], E[1] and the work arrays)
    const CpbSlab& L = a.lay;
    glbvt* s2 = (glbvt*)slab;
    const vt zero = T(0);
    const long z1 = L.z[1] / VN, e0 = L.e[0] / VN, e1 = L.e[1] / VN, end = L.stride / VN;
    if (m.warm) {
        if (zs != 0) {
            const long src = L.z[zs] / VN;
            for (long q = tid; q < z1; q += nthr) s2[q] = s2[src + q];
        }
        if (es != 0)
            for (long q = tid; q < e1 - e0; q += nthr) s2[e0 + q] = s2[e1 + q];
        __syncthreads();  // the copies have read Z[zs] and E[1] before they are cleared
        for (long q = z1 + tid; q < e0; q += nthr) s2[q] = zero;
        for (long q = e1 + tid; q < end; q += nthr) s2[q] = zero;
    } else {
        for (long q = tid; q < end; q += nthr) s2[q] = zero;
    }
    __syncthreads();  // x+ lands in ranges other lanes have just written
    if (tid < nx) {
        const T v = s_xp[tid];
        ((gl<T>*)slab)[L.z[0] + p.X0 + tid] = v;
        ((gl<T>*)slab)[L.x0 + tid] = v;
    }
    if (tid == 0) {
        _Pragma("unroll") for (int q = 0; q < 6; ++q) ctl->red[q] = 0;
        ctl->k = 0;
        ctl->done = 0;
        ctl->final_k = -1;
        ctl->flags = 0;
        ctl->pad = 0;
        a.done[b] = 0;
    }
    if constexpr (AA) {
        // G (64 doubles) and the state block behind it (cpa_layout_dims). The other arrays are not
        // cleared: cpa_body writes each of them before it sets the state field that lets it be
        // read. dg / dr are read in the committed slots only (`count` of them; the slot `head`
        // being pushed under `have` is taken from registers), pg / pr under `have`, sg under
        // `pending`; all three fields are zero from here on.
        typedef double v2 __attribute__((ext_vector_type(2)));
        typedef __attribute__((address_space(1))) v2 glbv2;
        const CpaSlab& A = aa->lay;
        glbv2* g2 = (glbv2*)(aa->slab + (size_t)b * A.stride + A.G);
        const long n2 = (A.state - A.G) / 2 + ((long)sizeof(CpaState) + 15) / 16;
        const v2 z2 = 0.0;
        for (long q = tid; q < n2; q += nthr) g2[q] = z2;
    }
}

template <class T>
__global__ void __launch_bounds__(kCpbBlock) k_mpc_step(Dev p, CpbArg a, MpcArg m) {
    mpc_step_body<T, false>(p, a, m, nullptr, nullptr);
}

__global__ void __launch_bounds__(kCpbBlock) k_mpc_step_aa(Dev p, CpbArg a, MpcArg m, CpaArg aa, int* counts) {
    mpc_step_body<double, true>(p, a, m, &aa, counts);
}

// elements of the shared tables (sqrt Q, sqrt R, sqrt Pf and the four box tables)
long tab_elems(const Dev& p) {
    return (long)p.nSQ * p.nx * p.nx + (long)p.nSR * p.nu * p.nu + (long)p.nSP * p.nx * p.nx +
           2L * p.nBnl * (p.nx + p.nu) + 2L * p.nBl * p.nx;
}

template <class T>
hipError_t cpb_launch_t(const Dev& p, const CpbArg& a, hipStream_t stream) {
    if (a.lds_tabs)
        k_cpb<T, true><<<a.B, kCpbBlock, tab_elems(p) * sizeof(T), stream>>>(p, a);
    else
        k_cpb<T, false><<<a.B, kCpbBlock, 0, stream>>>(p, a);
    return hipGetLastError();
}

}  // namespace

CpbSlab cpb_layout(const Dev& p, bool f32) {
    return cpb_layout_dims(p.P, p.D, p.n, p.m, p.nx, p.nu, f32 ? (int)sizeof(float) : (int)sizeof(double));
}

size_t cpb_tab_bytes(const Dev& p, bool f32) {
    const long b = tab_elems(p) * (long)(f32 ? sizeof(float) : sizeof(double));
    return b <= kCpbLdsTabs ? (size_t)b : 0;
}

hipError_t cpb_launch(const Dev& p, const CpbArg& a, bool f32, hipStream_t stream) {
    return f32 ? cpb_launch_t<float>(p, a, stream) : cpb_launch_t<double>(p, a, stream);
}

const char* cpb_name(bool f32, bool lds_tabs) {
    if (f32) return lds_tabs ? "k_cpb<float, true>" : "k_cpb<float, false>";
    return lds_tabs ? "k_cpb<true>" : "k_cpb<false>";
}

CpaSlab cpa_layout(const Dev& p, int m) { return cpa_layout_dims(p.P, p.D, m); }

hipError_t cpa_launch(const Dev& p, const CpbArg& a, const CpaArg& aa, hipStream_t stream) {
    if (a.lds_tabs)
        k_cpa<double, true><<<a.B, kCpbBlock, tab_elems(p) * sizeof(double), stream>>>(p, a, aa);
    else
        k_cpa<double, false><<<a.B, kCpbBlock, 0, stream>>>(p, a, aa);
    return hipGetLastError();
}

const char* cpa_name(bool lds_tabs) { return lds_tabs ? "k_cpa<true>" : "k_cpa<false>"; }

hipError_t mpc_step_launch(const Dev& p, const CpbArg& a, const MpcArg& m, bool f32, hipStream_t stream) {
    if (f32)
        k_mpc_step<float><<<a.B, kCpbBlock, 0, stream>>>(p, a, m);
    else
        k_mpc_step<double><<<a.B, kCpbBlock, 0, stream>>>(p, a, m);
    return hipGetLastError();
}

const char* mpc_step_name(bool f32) { return f32 ? "k_mpc_step<float>" : "k_mpc_step"; }

hipError_t mpc_step_aa_launch(const Dev& p, const CpbArg& a, const MpcArg& m, const CpaArg& aa, int* counts,
                              hipStream_t stream) {
    k_mpc_step_aa<<<a.B, kCpbBlock, 0, stream>>>(p, a, m, aa, counts);
    return hipGetLastError();
}

const char* mpc_step_aa_name() { return "k_mpc_step_aa"; }

}  // namespace raocp
