// raocp_eval.hip — the evaluation of a primal, as its own translation unit (host interface:
// raocp_eval.h; the AVaR routine and the sweep's launch plan: raocp_eval_ops.h).
//
// For a flat primal z and an initial state x0, with anc(j) the parent of j and ch(i) the
// children of i:
//   stage cost     l_j = |sqrtQ_j x_anc(j)|^2 + |sqrtR_j u_anc(j)|^2   (node j >= 1; what the SOC
//                  rows eta3 .. eta6 bound by tau_j, and what k_mpc_step records)
//   terminal cost  V_l = |sqrtPf_l x_l|^2                               (leaf l)
//   cost-to-go     V_i = AVaR_{alpha_i, cond}((l_j + V_j) for j in ch(i)), backwards by stage
//   objective      V_0; beside it s_0 (the primal's own epigraph value at the root),
//   box violation  max over every active box of max(lo - w, w - hi, 0), w = [x_i; u_i] / x_l
//   dynamics       max(|x_0 - x0|_inf, max_j |x_j - A_j x_anc(j) - B_j u_anc(j)|_inf)
//
// k_eval_nodes  node-parallel, one launch: a group of G lanes (8 .. 64, a power of two covering
//               max(nx, nu) where it can) takes one node, stages x_j, x_anc(j), u_anc(j) in LDS
//               as doubles and lets lane r take row r of the products (the L weights are
//               column-major M[k rows + r] and dW holds [B'; A'], so the lanes of a group read
//               consecutive addresses for every k). It writes w[j] = l_j (+ V_l for a leaf) and
//               val[j], and per workgroup the two maxima into part[].
// k_eval_sweep  the backward recursion, one parent per thread: val[i] = AVaR(w[ch(i)]),
//               w[i] += val[i]. One launch per stage while the stage has more parents than one
//               workgroup; the last launch runs every remaining stage in one workgroup with a
//               barrier between two stages, folds part[] and writes the four results.
// k_eval_batch  one workgroup per instance of a batch: the node pass over its slab's final
//               primal, then every stage with workgroup barriers; w[] in LDS when it fits.
// Stage order comes from launch order on one stream and from workgroup barriers only: no flag,
// counter, spin or atomic between workgroups, and every loop is bounded by a node, row, child or
// stage count. The maxima keep a NaN operand (nmax), and AVaR returns NaN for a NaN outcome, so
// a NaN anywhere in the primal reaches the results.
//
// Precision: values are loaded in the context's scalar type T and widened; every product, sum,
// the AVaR sweep and the maxima are double on a context of either precision.

#include "raocp_eval.h"

namespace raocp {
namespace {

template <class T>
using cg = const __attribute__((address_space(1))) T*;
typedef __attribute__((address_space(1))) const int glbi;

__host__ __device__ inline int eval_group(int nx, int nu) {
    const int need = nx > nu ? nx : nu;
    int G = 8;
    while (G < need && G < 64) G *= 2;
    return G;
}
// doubles of LDS a group stages per node: x_j, x_anc(j), u_anc(j)
__host__ __device__ inline int eval_stage_doubles(int nx, int nu) { return 2 * nx + nu; }

// sum over the G lanes of a group (G a power of two <= 64, groups aligned in the wave)
__device__ __forceinline__ double group_sum(double v, int G) {
    for (int off = G >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off, G);
    return v;
}

// the NaN-keeping maxima of a workgroup's lanes, valid in thread 0; red: 2 * (blockDim.x / 64) doubles
__device__ __forceinline__ void block_nmax2(double& a, double& b, ldsd* red) {
    for (int off = 32; off > 0; off >>= 1) {
        a = nmax(a, __shfl_xor(a, off));
        b = nmax(b, __shfl_xor(b, off));
    }
    const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[2 * wave] = a;
        red[2 * wave + 1] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int q = 1; q < nw; ++q) {
            a = nmax(a, red[2 * q]);
            b = nmax(b, red[2 * q + 1]);
        }
}

// One node j by a group of G lanes (lane l of the group; j >= n: the group idles but keeps the
// barriers and the shuffles). st: the group's staging rows. cost and vleaf are the group's sums
// (every lane holds them); box and dyn accumulate the lane's own maxima.
template <class T>
__device__ __forceinline__ void eval_node(const Dev& p, cg<T> z, cg<T> x0, int w_stride, int j, int l, int G, ldsd* st,
                                          double& cost, double& vleaf, double& box, double& dyn) {
    const int nx = p.nx, nu = p.nu;
    const bool on = j < p.n;
    ldsd* xj = st;
    ldsd* xa = st + nx;
    ldsd* ua = st + 2 * nx;
    const int a = (on && j > 0) ? ((glbi*)p.anc)[j] : 0;
    __syncthreads();  // the rows of the node before have been read
    if (on) {
        for (int k = l; k < nx; k += G) {
            xj[k] = (double)z[p.X0 + (long)j * nx + k];
            xa[k] = (double)z[p.X0 + (long)a * nx + k];
        }
        for (int k = l; k < nu; k += G) ua[k] = (double)z[p.U0 + (long)a * nu + k];
    }
    __syncthreads();
    double s = 0.0, sl = 0.0;
    if (on) {
        if (j > 0) {
            cg<T> SQ = (cg<T>)p.SQ + (size_t)((glbi*)p.iSQ)[j] * nx * nx;
            cg<T> SR = (cg<T>)p.SR + (size_t)((glbi*)p.iSR)[j] * nu * nu;
            const int kind = ((glbrec*)p.cinfo)[j].x;
            const glbd* W = (const glbd*)p.dW + (size_t)kind * (nx + nu) * w_stride;  // rows B' (nu), then A' (nx)
            for (int r = l; r < nx; r += G) {
                double q = 0.0, f = xj[r];
                for (int k = 0; k < nx; ++k) {
                    const double xk = xa[k];
                    q += (double)SQ[k * nx + r] * xk;
                    f -= W[(size_t)(nu + k) * w_stride + r] * xk;
                }
                for (int k = 0; k < nu; ++k) f -= W[(size_t)k * w_stride + r] * ua[k];
                s += q * q;
                dyn = nmax(dyn, fabs(f));
            }
            for (int r = l; r < nu; r += G) {
                double q = 0.0;
                for (int k = 0; k < nu; ++k) q += (double)SR[k * nu + r] * ua[k];
                s += q * q;
            }
        } else {
            for (int r = l; r < nx; r += G) dyn = nmax(dyn, fabs(xj[r] - (double)x0[r]));
        }
        if (j >= p.m) {
            cg<T> SP = (cg<T>)p.SP + (size_t)((glbi*)p.iSP)[j] * nx * nx;
            for (int r = l; r < nx; r += G) {
                double q = 0.0;
                for (int k = 0; k < nx; ++k) q += (double)SP[k * nx + r] * xj[k];
                sl += q * q;
            }
            const int ib = ((glbi*)p.iBl)[j];
            if (ib >= 0) {
                cg<T> lo = (cg<T>)p.blo_l + (size_t)ib * nx;
                cg<T> hi = (cg<T>)p.bhi_l + (size_t)ib * nx;
                for (int r = l; r < nx; r += G) {
                    const double w = xj[r];
                    box = nmax(box, nmax((double)lo[r] - w, w - (double)hi[r]));
                }
            }
        } else {
            const int ib = ((glbi*)p.iBnl)[j];
            if (ib >= 0) {
                cg<T> lo = (cg<T>)p.blo_nl + (size_t)ib * (nx + nu);
                cg<T> hi = (cg<T>)p.bhi_nl + (size_t)ib * (nx + nu);
                for (int r = l; r < nx + nu; r += G) {
                    const double w = r < nx ? (double)xj[r] : (double)z[p.U0 + (long)j * nu + (r - nx)];
                    box = nmax(box, nmax((double)lo[r] - w, w - (double)hi[r]));
                }
            }
        }
    }
    cost = group_sum(s, G);
    vleaf = group_sum(sl, G);
}

// val[i] = AVaR of the children's w, w[i] += val[i], for parent i
template <class T, class WP>
__device__ __forceinline__ double eval_parent(const Dev& p, WP w, int i) {
    const int c0 = ((glbi*)p.ch_start)[i], nc = ((glbi*)p.nch)[i];
    const double alpha = (double)((cg<T>)p.alpha_r)[i];
    return avar_ru(w + c0, (cg<T>)p.cond + c0, nc, alpha);
}

template <class T>
__global__ __launch_bounds__(kEvalBlock) void k_eval_nodes(Dev p, EvalArg a) {
    extern __shared__ __attribute__((aligned(16))) double smem_eval[];
    ldsd* sm = (ldsd*)smem_eval;
    const int G = eval_group(p.nx, p.nu), gpb = kEvalBlock / G;
    const int g = threadIdx.x / G, l = threadIdx.x % G;
    ldsd* red = sm;  // 2 * (kEvalBlock / 64) doubles
    ldsd* st = sm + 2 * (kEvalBlock / 64) + g * eval_stage_doubles(p.nx, p.nu);
    cg<T> z = (cg<T>)a.z;
    cg<T> x0 = (cg<T>)a.x0;
    glbd* w = (glbd*)a.w;
    glbd* val = (glbd*)a.val;
    double box = 0.0, dyn = 0.0;
    // every lane of the workgroup makes the same number of trips (base depends on the block only)
    for (int base = blockIdx.x * gpb; base < p.n; base += gridDim.x * gpb) {
        const int j = base + g;
        double cost, vleaf;
        eval_node<T>(p, z, x0, a.w_stride, j, l, G, st, cost, vleaf, box, dyn);
        if (l == 0 && j < p.n) {
            w[j] = cost + vleaf;
            val[j] = vleaf;
        }
    }
    __syncthreads();
    block_nmax2(box, dyn, red);
    if (threadIdx.x == 0) {
        ((glbd*)a.part)[2 * blockIdx.x] = box;
        ((glbd*)a.part)[2 * blockIdx.x + 1] = dyn;
    }
}

template <class T>
__global__ __launch_bounds__(kEvalSweepBlock) void k_eval_sweep(Dev p, EvalArg a, int s_hi, int s_lo, int last) {
    glbd* w = (glbd*)a.w;
    glbd* val = (glbd*)a.val;
    glbi* sp = (glbi*)p.stage_ptr;
    const int step = gridDim.x * kEvalSweepBlock;
    for (int t = s_hi; t >= s_lo; --t) {
        const int hi = sp[t + 1];
        for (int i = sp[t] + blockIdx.x * kEvalSweepBlock + threadIdx.x; i < hi; i += step) {
            const double v = eval_parent<T>(p, (const glbd*)w, i);
            val[i] = v;
            w[i] += v;
        }
        if (t > s_lo) __syncthreads();  // more than one stage: the launch is one workgroup
    }
    if (!last) return;
    __syncthreads();
    // the workgroup is one wave: fold the node pass's partial maxima
    double box = 0.0, dyn = 0.0;
    for (int q = threadIdx.x; q < a.grid; q += kEvalSweepBlock) {
        box = nmax(box, ((const glbd*)a.part)[2 * q]);
        dyn = nmax(dyn, ((const glbd*)a.part)[2 * q + 1]);
    }
    for (int off = 32; off > 0; off >>= 1) {
        box = nmax(box, __shfl_xor(box, off));
        dyn = nmax(dyn, __shfl_xor(dyn, off));
    }
    if (threadIdx.x == 0) {
        glbd* out = (glbd*)a.out;
        out[0] = val[0];
        out[1] = (double)((cg<T>)a.z)[p.S0];
        out[2] = box;
        out[3] = dyn;
    }
}

// LDSW: the instance's work array w[n] is in LDS (else in its row of a.scratch)
template <class T, bool LDSW>
__global__ __launch_bounds__(kEvalBlock) void k_eval_batch(Dev p, EvalBatchArg a) {
    extern __shared__ __attribute__((aligned(16))) double smem_eval[];
    ldsd* sm = (ldsd*)smem_eval;
    const int b = blockIdx.x;
    if (b >= a.B) return;
    const int G = eval_group(p.nx, p.nu), gpb = kEvalBlock / G;
    const int g = threadIdx.x / G, l = threadIdx.x % G;
    ldsd* red = sm;
    ldsd* st = sm + 2 * (kEvalBlock / 64) + g * eval_stage_doubles(p.nx, p.nu);
    ldsd* wl = sm + 2 * (kEvalBlock / 64) + gpb * eval_stage_doubles(p.nx, p.nu);
    glbd* wg = (glbd*)a.scratch + (LDSW ? 0 : (size_t)b * p.n);
    cg<T> slab = (cg<T>)a.slab + (size_t)b * a.lay.stride;
    cg<T> z = slab + a.lay.z[((glbi*)a.zsel)[b]];
    cg<T> x0 = slab + a.lay.x0;
    double box = 0.0, dyn = 0.0;
    for (int base = 0; base < p.n; base += gpb) {
        const int j = base + g;
        double cost, vleaf;
        eval_node<T>(p, z, x0, a.w_stride, j, l, G, st, cost, vleaf, box, dyn);
        if (l == 0 && j < p.n) {
            if (LDSW) wl[j] = cost + vleaf;
            else wg[j] = cost + vleaf;
        }
    }
    glbi* sp = (glbi*)p.stage_ptr;
    for (int t = p.N - 1; t >= 0; --t) {
        __syncthreads();  // the stage below (the node pass before the first) is complete
        const int hi = sp[t + 1];
        for (int i = sp[t] + threadIdx.x; i < hi; i += kEvalBlock) {
            if (LDSW) wl[i] += eval_parent<T>(p, (const ldsd*)wl, i);
            else wg[i] += eval_parent<T>(p, (const glbd*)wg, i);
        }
    }
    __syncthreads();
    block_nmax2(box, dyn, red);
    if (threadIdx.x == 0) {
        glbd* out = (glbd*)a.out + 4 * (size_t)b;
        out[0] = LDSW ? wl[0] : wg[0];  // l_0 = 0: w[0] is V_0
        out[1] = (double)z[p.S0];
        out[2] = box;
        out[3] = dyn;
    }
}

size_t eval_lds_bytes(const Dev& p) {
    const int gpb = kEvalBlock / eval_group(p.nx, p.nu);
    return (size_t)(2 * (kEvalBlock / 64) + gpb * eval_stage_doubles(p.nx, p.nu)) * sizeof(double);
}

template <class T>
hipError_t eval_launch_t(const Dev& p, const EvalArg& a, const std::vector<EvalLaunch>& plan, hipStream_t stream) {
    k_eval_nodes<T><<<a.grid, kEvalBlock, eval_lds_bytes(p), stream>>>(p, a);
    for (const EvalLaunch& L : plan)
        k_eval_sweep<T><<<L.blocks, kEvalSweepBlock, 0, stream>>>(p, a, L.s_hi, L.s_lo, L.last ? 1 : 0);
    return hipGetLastError();
}

template <class T>
hipError_t eval_batch_launch_t(const Dev& p, const EvalBatchArg& a, hipStream_t stream) {
    const bool ldsw = eval_batch_w_in_lds(p);
    const size_t lds = eval_lds_bytes(p) + (ldsw ? (size_t)p.n * sizeof(double) : 0);
    if (ldsw) k_eval_batch<T, true><<<a.B, kEvalBlock, lds, stream>>>(p, a);
    else k_eval_batch<T, false><<<a.B, kEvalBlock, lds, stream>>>(p, a);
    return hipGetLastError();
}

}  // namespace

int eval_nodes_grid(const Dev& p) {
    const int gpb = kEvalBlock / eval_group(p.nx, p.nu);
    const int g = (p.n + gpb - 1) / gpb;
    return g < 1 ? 1 : (g > kEvalMaxGrid ? kEvalMaxGrid : g);
}

hipError_t eval_launch(const Dev& p, const EvalArg& a, const std::vector<EvalLaunch>& plan, bool f32,
                       hipStream_t stream) {
    return f32 ? eval_launch_t<float>(p, a, plan, stream) : eval_launch_t<double>(p, a, plan, stream);
}

std::string eval_name(bool f32, int sweeps) {
    const std::string T = f32 ? "float" : "double";
    return "k_eval_nodes<" + T + "> + k_eval_sweep<" + T + "> x" + std::to_string(sweeps);
}

bool eval_batch_w_in_lds(const Dev& p) { return (size_t)p.n * sizeof(double) <= (size_t)kEvalBatchLdsW; }

hipError_t eval_batch_launch(const Dev& p, const EvalBatchArg& a, bool f32, hipStream_t stream) {
    return f32 ? eval_batch_launch_t<float>(p, a, stream) : eval_batch_launch_t<double>(p, a, stream);
}

const char* eval_batch_name(bool f32) { return f32 ? "k_eval_batch<float>" : "k_eval_batch<double>"; }

}  // namespace raocp
