// raocp_batch.hip — the host code of the batched solves (raocp_cp_batch_*), the closed-loop
// simulation of a batch (raocp_cp_batch_mpc, raocp_cp_batch_mpc_aa) and the evaluation of a primal (raocp_evaluate,
// raocp_cp_batch_evaluate). Host code only: it launches through raocp_cpb.h and raocp_eval.h
// (the kernels are in raocp_cpb.hip and raocp_eval.hip) and falls back on the public single-solve
// entry points of raocp_capi.hip, so it compiles without the kernel families of that unit.

#include <algorithm>
#include <cmath>
#include <limits>
#include <string>
#include <vector>

#include "raocp_host.h"

// k_cpb (raocp_cpb.hip) covers this context's batched solves: unsharded, sizes within the
// kernel's limits; RAOCP_CPB=0 (read at call time) selects the sequential solves. An fp64
// context takes the kernel by default. An fp32 context keeps the sequential solves it has always
// run unless RAOCP_CPB_F32=1 (read at call time) asks for the float form, which reads the fp32
// tables of the context's per-stage dynamics (an fp32 context always holds them).
bool raocp::cpb_on(const raocp_ctx* c) {
    const char* e = getenv("RAOCP_CPB");
    if (e && e[0] == '0') return false;
    if (c->f32) {
        const char* f = getenv("RAOCP_CPB_F32");
        if (!(f && f[0] == '1')) return false;
        if (!(c->W2 && c->RG2 && c->KM2 && c->F2)) return false;
    }
    return !c->comm && c->sh_R == 1 && c->nx <= raocp::kCpbMaxNx && c->nu <= raocp::kCpbMaxNu;
}
void raocp::batch_free(raocp_ctx* c) {
    auto& bt = c->bt;
    for (void* p : {(void*)bt.slab, (void*)bt.ctl, (void*)bt.done, (void*)bt.hist, (void*)bt.u0, (void*)bt.aslab, (void*)bt.alog})
        if (p) (void)hipFree(p);
    bt.aslab = bt.alog = nullptr;
    bt.a_m = 0;
    bt.a_rows = 0;
    bt.slab = nullptr;
    bt.hist = bt.u0 = nullptr;
    bt.ctl = nullptr;
    bt.done = nullptr;
    bt.cap_B = 0;
    bt.hist_rows = 0;
}
void raocp::mpc_free(raocp_ctx* c) {
    if (c->mpc_buf) (void)hipFree(c->mpc_buf);
    c->mpc_buf = nullptr;
    c->mpc_cap = 0;
}

// ---- evaluation of a primal (raocp_evaluate, raocp_cp_batch_evaluate; raocp_eval.hip)

int raocp::eval_ensure(raocp_ctx* c) {
    if (c->eval_buf) return RAOCP_OK;
    c->eval_plan = raocp::eval_sweep_plan(c->stage_ptr);
    c->eval_grid = raocp::eval_nodes_grid(c->dev);
    return c->alloc(&c->eval_buf, (size_t)2 * c->n + (size_t)2 * c->eval_grid + RAOCP_EVAL_N + c->nx);
}

// the single-solve kernels over a device primal and a device initial state of the context's
// scalar type; the four results (and V_i of every node) to the host
raocp::EvalArg raocp::eval_arg(raocp_ctx* c, const void* dz, const void* dx0) {
    raocp::EvalArg a{};
    a.z = dz;
    a.x0 = dx0;
    a.w = c->eval_buf;
    a.val = a.w + c->n;
    a.part = a.val + c->n;
    a.out = a.part + (size_t)2 * c->eval_grid;
    a.grid = c->eval_grid;
    a.w_stride = raocp::tstride(c->KP);
    return a;
}

namespace {

double* eval_x0_slot(raocp_ctx* c) { return c->eval_buf + (size_t)2 * c->n + (size_t)2 * c->eval_grid + RAOCP_EVAL_N; }

int eval_run(raocp_ctx* c, const void* dz, const void* dx0, double* out, double* node_values) {
    const raocp::EvalArg a = eval_arg(c, dz, dx0);
    HIPCHK(raocp::eval_launch(c->dev, a, c->eval_plan, c->f32, c->stream));
    HIPCHK(hipMemcpyAsync(out, a.out, RAOCP_EVAL_N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (node_values)
        HIPCHK(hipMemcpyAsync(node_values, a.val, (size_t)c->n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return RAOCP_OK;
}

// every instance of a batch k_cpb ran, inside the slabs: one launch
int batch_eval_kernel(raocp_ctx* c, double* out) {
    const auto& bt = c->bt;
    const int B = bt.B;
    const bool ldsw = raocp::eval_batch_w_in_lds(c->dev);
    const size_t n_out = (size_t)B * RAOCP_EVAL_N, n_scr = ldsw ? 0 : (size_t)B * c->n;
    DevMem blk;  // [out | scratch | zsel]
    HIPCHK(blk.alloc((n_out + n_scr) * sizeof(double) + (size_t)B * sizeof(int)));
    std::vector<int> zsel(B);
    for (int b = 0; b < B; ++b) zsel[b] = (bt.fk[b] + 1) % 3;  // the primal raocp_cp_batch_get reads
    raocp::EvalBatchArg a{};
    a.slab = bt.slab;
    a.lay = bt.lay;
    a.out = (double*)blk.p;
    a.scratch = a.out + n_out;
    a.zsel = (const int*)(a.scratch + n_scr);
    a.B = B;
    a.w_stride = raocp::tstride(c->KP);
    hipError_t e = hipMemcpyAsync((void*)a.zsel, zsel.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = raocp::eval_batch_launch(c->dev, a, c->f32, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, a.out, n_out * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(RAOCP_ERR_HIP, std::string("batch evaluation: ") + hipGetErrorString(e));
    return RAOCP_OK;
}

// every instance of a batch that ran as sequential solves: the single-solve kernels over each
// stored final primal (staged in tmpP; the context's iterate and initial state are not touched)
int batch_eval_seq(raocp_ctx* c, double* out) {
    const auto& bt = c->bt;
    if (bt.hx0.size() != (size_t)bt.B * c->nx || bt.hz.size() != (size_t)bt.B * c->P)
        return fail(RAOCP_ERR_STATE, "the last batch kept no final primals");
    int rc;
    if ((rc = eval_ensure(c))) return rc;
    for (int b = 0; b < bt.B; ++b) {
        if ((rc = copy_in(c, c->tmpP, bt.hz.data() + (size_t)b * c->P, (size_t)c->P, 0))) return rc;
        if ((rc = copy_in(c, eval_x0_slot(c), bt.hx0.data() + (size_t)b * c->nx, (size_t)c->nx, 0))) return rc;
        if ((rc = eval_run(c, c->tmpP, eval_x0_slot(c), out + (size_t)b * RAOCP_EVAL_N, nullptr))) return rc;
    }
    return RAOCP_OK;
}

// ---- batched solves (raocp_cp_batch_run, raocp_cp_batch_run_aa)

int batch_chunk() {
    const int v = env_int("RAOCP_BATCH_CHUNK", 256);
    return v >= 1 ? v : 256;
}

// the device buffers of a batch of B instances with `rows` history rows each
int batch_ensure(raocp_ctx* c, int B, size_t rows) {
    auto& bt = c->bt;
    if (bt.cap_B == B && rows <= bt.hist_rows) return RAOCP_OK;
    const size_t want = std::max(rows, bt.cap_B == B ? bt.hist_rows : (size_t)0);
    batch_free(c);
    bt.lay = raocp::cpb_layout(c->dev, c->f32);
    HIPCHK(hipMalloc((void**)&bt.slab, (size_t)B * bt.lay.stride * c->wsz));
    HIPCHK(hipMalloc((void**)&bt.ctl, (size_t)B * sizeof(Ctl)));
    HIPCHK(hipMalloc((void**)&bt.done, (size_t)B * sizeof(int)));
    HIPCHK(hipMalloc((void**)&bt.hist, (size_t)B * want * 6 * sizeof(double)));
    HIPCHK(hipMalloc((void**)&bt.u0, (size_t)B * c->nu * sizeof(double)));
    bt.cap_B = B;
    bt.hist_rows = want;
    return RAOCP_OK;
}

// rows of `width` host doubles, one per instance, into the slabs at element offset `off` (an
// fp32 context converts on the host, as copy_in does)
int batch_scatter(raocp_ctx* c, long off, const double* src, size_t width, int B) {
    const size_t w = (size_t)c->wsz;
    char* dst = c->bt.slab + (size_t)off * w;
    if (c->f32) {
        const std::vector<float> tmp(src, src + width * (size_t)B);
        HIPCHK(hipMemcpy2DAsync(dst, (size_t)c->bt.lay.stride * w, tmp.data(), width * w, width * w, (size_t)B,
                                hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return RAOCP_OK;
    }
    HIPCHK(hipMemcpy2DAsync(dst, (size_t)c->bt.lay.stride * w, src, width * w, width * w, (size_t)B, hipMemcpyHostToDevice,
                            c->stream));
    return RAOCP_OK;
}

// the kernel arguments of a batch of B instances with `rows` history rows each
raocp::CpbArg batch_arg(raocp_ctx* c, int B, size_t rows) {
    auto& bt = c->bt;
    raocp::CpbArg a{};
    a.slab = bt.slab;
    a.lay = bt.lay;
    a.ctl = bt.ctl;
    a.done = bt.done;
    a.hist = bt.hist;
    a.hist_rows = (long)rows;
    a.u0 = bt.u0;
    a.B = B;
    a.chunk = batch_chunk();
    a.lds_tabs = raocp::cpb_tab_bytes(c->dev, c->f32) > 0 ? 1 : 0;
    if (c->f32) {
        a.W2 = c->W2;
        a.RG2 = c->RG2;
        a.KM2 = c->KM2;
        a.F2 = c->F2;
    }
    return a;
}

// the start of a batch on the device: the buffers of B instances with `rows` history rows, the
// slabs, done and u0 cleared, the starting iterates (z0 with eta0, or none), x0 and one control
// block per instance (hc: the caller's host copy, which outlives the asynchronous upload)
int batch_start(raocp_ctx* c, int B, size_t rows, const double* x0, const double* z0, const double* eta0, int max_iters,
                double tol, double alpha, std::vector<Ctl>& hc) {
    auto& bt = c->bt;
    int rc;
    if ((rc = batch_ensure(c, B, rows))) return rc;
    const raocp::CpbSlab& L = bt.lay;
    HIPCHK(hipMemsetAsync(bt.slab, 0, (size_t)B * L.stride * c->wsz, c->stream));
    HIPCHK(hipMemsetAsync(bt.done, 0, (size_t)B * sizeof(int), c->stream));
    HIPCHK(hipMemsetAsync(bt.u0, 0, (size_t)B * c->nu * sizeof(double), c->stream));
    if (z0) {
        if ((rc = batch_scatter(c, L.z[0], z0, (size_t)c->P, B))) return rc;
        if ((rc = batch_scatter(c, L.e[0], eta0, (size_t)c->D, B))) return rc;
    }
    // x0 into node 0's state (cache_initial_state) and as the projection's x0bar
    if ((rc = batch_scatter(c, L.z[0] + c->dev.X0, x0, (size_t)c->nx, B))) return rc;
    if ((rc = batch_scatter(c, L.x0, x0, (size_t)c->nx, B))) return rc;
    Ctl h{};
    h.alpha = alpha;
    h.final_k = -1;
    h.max_iters = max_iters;
    h.tol = tol;
    hc.assign((size_t)B, h);
    HIPCHK(hipMemcpyAsync(bt.ctl, hc.data(), hc.size() * sizeof(Ctl), hipMemcpyHostToDevice, c->stream));
    return RAOCP_OK;
}

// one solve of the batch: `launch` (k_cpb or k_cpa, a.chunk iterations each) until the done
// words, polled after every launch, say that every instance has finished
template <class F>
int batch_solve(raocp_ctx* c, const raocp::CpbArg& a, size_t rows, F launch) {
    std::vector<int> hd((size_t)a.B, 0);
    const long launches = (long)(rows + a.chunk - 1) / a.chunk + 1;  // every instance ends within rows iterations
    bool all = false;
    for (long l = 0; l < launches && !all; ++l) {
        if (int rc = launch()) return rc;
        HIPCHK(hipMemcpyAsync(hd.data(), a.done, hd.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        all = std::all_of(hd.begin(), hd.end(), [](int v) { return v != 0; });
    }
    if (!all) return fail(RAOCP_ERR_STATE, "batched CP kernel: an instance did not finish");
    return RAOCP_OK;
}

// the options of an accelerated batch (raocp_cp_batch_run_aa)
struct AaOpt {
    int m, every;
    double reg, safeguard;
};

// the acceleration's slabs and log for the batch buffers batch_ensure has just sized; cleared,
// so every instance starts with an empty history
int batch_ensure_aa(raocp_ctx* c, int B, int m) {
    auto& bt = c->bt;
    if (bt.a_m != m || bt.a_rows != bt.hist_rows) {
        if (bt.aslab) (void)hipFree(bt.aslab);
        if (bt.alog) (void)hipFree(bt.alog);
        bt.aslab = bt.alog = nullptr;
        bt.a_m = 0;
        bt.alay = raocp::cpa_layout(c->dev, m);
        HIPCHK(hipMalloc((void**)&bt.aslab, (size_t)B * bt.alay.stride * sizeof(double)));
        HIPCHK(hipMalloc((void**)&bt.alog, (size_t)B * bt.hist_rows * raocp::kAaRec * sizeof(double)));
        bt.a_m = m;
        bt.a_rows = bt.hist_rows;
    }
    HIPCHK(hipMemsetAsync(bt.aslab, 0, (size_t)B * bt.alay.stride * sizeof(double), c->stream));
    return RAOCP_OK;
}

// k_cpa's arguments over the buffers batch_ensure_aa has sized
raocp::CpaArg batch_aa_arg(raocp_ctx* c, const AaOpt& aa) {
    raocp::CpaArg ca{};
    ca.slab = c->bt.aslab;
    ca.lay = c->bt.alay;
    ca.log = c->bt.alog;
    ca.every = aa.every;
    ca.reg = aa.reg;
    ca.safeguard = aa.safeguard;
    return ca;
}

// the checks of an accelerated call, in the order raocp_cp_batch_run_aa has always made them: the
// options (RAOCP_ERR_ARG) ...
int aa_check_opt(const AaOpt& aa) {
    if (aa.m < 1 || aa.m > raocp::kAaMaxM) return fail(RAOCP_ERR_ARG, "accel must be in 1 .. 8");
    if (aa.every < 1) return fail(RAOCP_ERR_ARG, "accel_every must be >= 1");
    if (!(aa.reg >= 0.0) || !(aa.safeguard >= 0.0)) return fail(RAOCP_ERR_ARG, "accel_reg and accel_safeguard must be >= 0");
    return RAOCP_OK;
}
// ... and, after the sharded-context check of the plain call, the context (RAOCP_ERR_STATE)
int aa_check_ctx(const raocp_ctx* c) {
    if (c->f32) return fail(RAOCP_ERR_STATE, "accelerated batched solves are not available on an fp32 context");
    if (!cpb_on(c)) return fail(RAOCP_ERR_STATE, "accelerated batched solves need the batch kernel, which does not cover this context");
    return RAOCP_OK;
}

// aa: nullptr runs k_cpb; else k_cpa with these options
int batch_run_kernel(raocp_ctx* c, int B, const double* x0, const double* z0, const double* eta0, int max_iters,
                     double tol, double alpha, int* status, int* iters, double* err_hist, double* delta_hist,
                     const AaOpt* aa) {
    auto& bt = c->bt;
    const size_t rows = (size_t)max_iters + 1;
    int rc;
    bt.accel = false;
    std::vector<Ctl> hc;
    if ((rc = batch_start(c, B, rows, x0, z0, eta0, max_iters, tol, alpha, hc))) return rc;
    if (aa && (rc = batch_ensure_aa(c, B, aa->m))) return rc;
    const raocp::CpbArg a = batch_arg(c, B, rows);
    const raocp::CpaArg ca = aa ? batch_aa_arg(c, *aa) : raocp::CpaArg{};
    rc = batch_solve(c, a, rows, [&]() -> int {
        HIPCHK(aa ? raocp::cpa_launch(c->dev, a, ca, c->stream) : raocp::cpb_launch(c->dev, a, c->f32, c->stream));
        return RAOCP_OK;
    });
    if (rc) return rc;
    HIPCHK(hipMemcpy(hc.data(), bt.ctl, hc.size() * sizeof(Ctl), hipMemcpyDeviceToHost));
    std::vector<double> hh((size_t)B * rows * 6);
    HIPCHK(hipMemcpy(hh.data(), bt.hist, hh.size() * sizeof(double), hipMemcpyDeviceToHost));
    bt.fk.assign(B, 0);
    for (int b = 0; b < B; ++b) {
        const int fk = hc[b].final_k;
        bt.fk[b] = fk;
        iters[b] = fk + 1;
        status[b] = (hc[b].flags & 1) ? 2 : (fk < max_iters ? 0 : 1);
        for (int k = 0; k <= fk; ++k)
            for (int q = 0; q < 3; ++q) {
                const size_t s = ((size_t)b * rows + k) * 6;
                err_hist[((size_t)b * rows + k) * 3 + q] = hh[s + q];
                delta_hist[((size_t)b * rows + k) * 3 + q] = hh[s + 3 + q];
            }
    }
    bt.B = B;
    bt.kernel = true;
    bt.accel = aa != nullptr;
    bt.a_log_rows = rows;
    return RAOCP_OK;
}

// the fallback of a context k_cpb does not cover: the B solves one after another through the
// context's own loop, the context's iterate and initial state saved and put back
int batch_run_seq(raocp_ctx* c, int B, const double* x0, const double* z0, const double* eta0, int max_iters,
                  double tol, double alpha, int* status, int* iters, double* err_hist, double* delta_hist) {
    auto& bt = c->bt;
    const size_t rows = (size_t)max_iters + 1;
    double* const sz = c->cur_z;
    double* const se = c->cur_e;
    const bool had_x0 = c->has_x0;
    const std::vector<double> sx0 = c->h_x0;
    DevMem kz, ke;
    HIPCHK(kz.alloc((size_t)c->P * c->wsz + 64));
    if (ke.alloc((size_t)c->D * c->wsz + 64) != hipSuccess) return fail(RAOCP_ERR_HIP, "hipMalloc: batch fallback");
    (void)hipMemcpyAsync(kz.p, sz, (size_t)c->P * c->wsz, hipMemcpyDeviceToDevice, c->stream);
    (void)hipMemcpyAsync(ke.p, se, (size_t)c->D * c->wsz, hipMemcpyDeviceToDevice, c->stream);
    (void)hipStreamSynchronize(c->stream);
    bt.hz.assign((size_t)B * c->P, 0.0);
    bt.he.assign((size_t)B * c->D, 0.0);
    bt.hu0.assign((size_t)B * c->nu, 0.0);
    bt.hx0.assign(x0, x0 + (size_t)B * c->nx);
    bt.fk.assign(B, 0);
    int rc = RAOCP_OK;
    for (int b = 0; b < B && rc == RAOCP_OK; ++b) {
        if (z0) {
            if ((rc = raocp_set_primal(c, z0 + (size_t)b * c->P, 0))) break;
            if ((rc = raocp_set_dual(c, eta0 + (size_t)b * c->D, 0))) break;
        } else if ((rc = raocp_reset_iterate(c))) {
            break;
        }
        rc = raocp_cp_run(c, x0 + (size_t)b * c->nx, max_iters, tol, alpha, &status[b], &iters[b],
                          err_hist + (size_t)b * rows * 3, delta_hist + (size_t)b * rows * 3);
        if (rc == RAOCP_ERR_NAN_IN_BOX) {
            status[b] = 2;
            rc = RAOCP_OK;
        }
        if (rc) break;
        bt.fk[b] = iters[b] - 1;
        if ((rc = raocp_get_primal(c, bt.hz.data() + (size_t)b * c->P, 0))) break;
        if ((rc = raocp_get_dual(c, bt.he.data() + (size_t)b * c->D, 0))) break;
        for (int r = 0; r < c->nu; ++r) bt.hu0[(size_t)b * c->nu + r] = bt.hz[(size_t)b * c->P + c->dev.U0 + r];
    }
    const std::string msg = raocp::g_err;
    c->cur_z = sz;
    c->cur_e = se;
    (void)hipMemcpyAsync(sz, kz.p, (size_t)c->P * c->wsz, hipMemcpyDeviceToDevice, c->stream);
    (void)hipMemcpyAsync(se, ke.p, (size_t)c->D * c->wsz, hipMemcpyDeviceToDevice, c->stream);
    (void)hipStreamSynchronize(c->stream);
    if (had_x0) (void)raocp_set_initial_state(c, sx0.data());
    else c->has_x0 = false;
    if (rc) return fail(rc, msg);
    bt.B = B;
    bt.kernel = false;
    return RAOCP_OK;
}

// raocp_cp_batch_run (aa == nullptr) and raocp_cp_batch_run_aa: the checks in the order the two
// entry points have always made them, then the kernel or the sequential solves
int batch_run(raocp_ctx* c, int B, const double* x0, const double* z0, const double* eta0, int max_iters, double tol,
              double alpha, int* status, int* iters, double* err_hist, double* delta_hist, const AaOpt* aa) {
    DevGuard dg_(c);
    if (!c || !x0 || !status || !iters || !err_hist || !delta_hist) return fail(RAOCP_ERR_ARG, "null argument");
    if (B < 1 || B > 4096) return fail(RAOCP_ERR_ARG, "batch size must be in 1 .. 4096");
    if ((z0 == nullptr) != (eta0 == nullptr)) return fail(RAOCP_ERR_ARG, "z0 and eta0 are given together");
    if (max_iters < 0) return fail(RAOCP_ERR_ARG, "max_iters must be >= 0");
    int rc;
    if (aa && (rc = aa_check_opt(*aa))) return rc;
    if (c->comm || c->sh_R != 1) return fail(RAOCP_ERR_STATE, "batched solves are not available on a sharded context");
    if (aa && (rc = aa_check_ctx(c))) return rc;
    c->bt.B = 0;
    c->bt.accel = false;
    if (aa || cpb_on(c)) return batch_run_kernel(c, B, x0, z0, eta0, max_iters, tol, alpha, status, iters, err_hist, delta_hist, aa);
    return batch_run_seq(c, B, x0, z0, eta0, max_iters, tol, alpha, status, iters, err_hist, delta_hist);
}

// instance b's iterate of the last batch: the final one, or (prev) the one iteration final_k
// read: it read Z[final_k % 3], E[final_k % 2] and wrote the other buffers
int batch_get(raocp_ctx* c, int b, double* z, double* eta, bool prev) {
    DevGuard dg_(c);
    if (!c || !z || !eta) return fail(RAOCP_ERR_ARG, "null argument");
    const auto& bt = c->bt;
    if (bt.B < 1) return fail(RAOCP_ERR_STATE, "no batch has been run");
    if (b < 0 || b >= bt.B) return fail(RAOCP_ERR_ARG, "instance index out of range");
    if (!bt.kernel) {
        if (prev) return fail(RAOCP_ERR_STATE, "the sequential solves keep no previous iterate");
        std::copy(bt.hz.begin() + (size_t)b * c->P, bt.hz.begin() + (size_t)(b + 1) * c->P, z);
        std::copy(bt.he.begin() + (size_t)b * c->D, bt.he.begin() + (size_t)(b + 1) * c->D, eta);
        return RAOCP_OK;
    }
    // the slab holds the context's scalar type; an fp32 context widens on the host (copy_out)
    const size_t w = (size_t)c->wsz;
    const char* slab = bt.slab + (size_t)b * bt.lay.stride * w;
    const int k = bt.fk[b] + (prev ? 0 : 1);
    int rc;
    if ((rc = copy_out(c, z, (const double*)(slab + (size_t)bt.lay.z[k % 3] * w), (size_t)c->P, 0))) return rc;
    return copy_out(c, eta, (const double*)(slab + (size_t)bt.lay.e[k % 2] * w), (size_t)c->D, 0);
}

// ---- closed-loop simulation of a batch (raocp_cp_batch_mpc, raocp_cp_batch_mpc_aa)

// the per-step records on the device, as k_mpc_step takes them: one block, every array on a
// 256-B boundary; counts (an accelerated simulation only): [B][T][kAaCounts] ints behind them
int mpc_ensure(raocp_ctx* c, int B, int T, raocp::MpcArg* mb, int** counts) {
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t o = at;
        at += (bytes + 255) / 256 * 256;
        return o;
    };
    const size_t BT = (size_t)B * T;
    const size_t o_scen = take(BT * sizeof(int)), o_frz = take((size_t)B * sizeof(int));
    const size_t o_X = take((size_t)B * (T + 1) * c->nx * sizeof(double)), o_U = take(BT * c->nu * sizeof(double));
    const size_t o_cost = take(BT * sizeof(double)), o_status = take(BT * sizeof(int)), o_iters = take(BT * sizeof(int));
    const size_t o_err = take(BT * 3 * sizeof(double));
    const size_t o_cnt = counts ? take(BT * raocp::kAaCounts * sizeof(int)) : 0;
    if (at > c->mpc_cap) {
        mpc_free(c);
        HIPCHK(hipMalloc(&c->mpc_buf, at));
        c->mpc_cap = at;
    }
    char* base = (char*)c->mpc_buf;
    mb->scen = (int*)(base + o_scen);
    mb->frz = (int*)(base + o_frz);
    mb->X = (double*)(base + o_X);
    mb->U = (double*)(base + o_U);
    mb->cost = (double*)(base + o_cost);
    mb->status = (int*)(base + o_status);
    mb->iters = (int*)(base + o_iters);
    mb->err = (double*)(base + o_err);
    if (counts) *counts = (int*)(base + o_cnt);
    return RAOCP_OK;
}

// final_k of every instance's last solve: the last step with iterations (a frozen instance's
// slab keeps the solve that froze it)
void mpc_final_k(std::vector<int>& fk, int B, int T, const int* iters) {
    fk.assign(B, 0);
    for (int b = 0; b < B; ++b)
        for (int t = T - 1; t >= 0; --t)
            if (iters[(size_t)b * T + t] > 0) {
                fk[b] = iters[(size_t)b * T + t] - 1;
                break;
            }
}

// the loop on the device: per step the chunked k_cpb launches with their done poll, then one
// k_mpc_step launch; nothing else crosses the host boundary inside the T loop. aa: nullptr runs
// k_cpb and k_mpc_step; else k_cpa with these options and k_mpc_step_aa, which fills aa_counts and
// empties the acceleration's state on the device (the slabs and the log are sized and cleared
// once, before the loop)
int batch_mpc_kernel(raocp_ctx* c, int B, int T, const double* x0, const int* scen, int max_iters, double tol,
                     double alpha, int warm, double* X, double* U, double* cost, int* status, int* iters, double* err,
                     const AaOpt* aa, int* aa_counts) {
    auto& bt = c->bt;
    const size_t rows = (size_t)max_iters + 1, BT = (size_t)B * T;
    int rc;
    if (c->h_mpc_ab.empty()) return fail(RAOCP_ERR_STATE, "no plant tables for the root's children");
    if (!c->d_mpc_ab && (rc = upload_t(c, &c->d_mpc_ab, c->h_mpc_ab))) return rc;
    std::vector<Ctl> hc;
    if ((rc = batch_start(c, B, rows, x0, nullptr, nullptr, max_iters, tol, alpha, hc))) return rc;
    if (aa && (rc = batch_ensure_aa(c, B, aa->m))) return rc;
    raocp::MpcArg m{};
    int* d_counts = nullptr;
    if ((rc = mpc_ensure(c, B, T, &m, aa ? &d_counts : nullptr))) return rc;
    HIPCHK(hipMemsetAsync(m.frz, 0xff, (size_t)B * sizeof(int), c->stream));  // -1: running
    HIPCHK(hipMemcpyAsync((void*)m.scen, scen, BT * sizeof(int), hipMemcpyHostToDevice, c->stream));
    const raocp::CpbArg a = batch_arg(c, B, rows);
    const raocp::CpaArg ca = aa ? batch_aa_arg(c, *aa) : raocp::CpaArg{};
    m.ab = c->d_mpc_ab;
    m.T = T;
    m.warm = warm ? 1 : 0;
    for (int t = 0; t < T; ++t) {
        rc = batch_solve(c, a, rows, [&]() -> int {
            HIPCHK(aa ? raocp::cpa_launch(c->dev, a, ca, c->stream) : raocp::cpb_launch(c->dev, a, c->f32, c->stream));
            return RAOCP_OK;
        });
        if (rc) return rc;
        m.t = t;
        m.last = t == T - 1 ? 1 : 0;
        HIPCHK(aa ? raocp::mpc_step_aa_launch(c->dev, a, m, ca, d_counts, c->stream)
                  : raocp::mpc_step_launch(c->dev, a, m, c->f32, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(X, m.X, (size_t)B * (T + 1) * c->nx * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(U, m.U, BT * c->nu * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(cost, m.cost, BT * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(status, m.status, BT * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(iters, m.iters, BT * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(err, m.err, BT * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (aa) HIPCHK(hipMemcpy(aa_counts, d_counts, BT * raocp::kAaCounts * sizeof(int), hipMemcpyDeviceToHost));
    mpc_final_k(bt.fk, B, T, iters);
    bt.B = B;
    bt.kernel = true;
    bt.accel = aa != nullptr;  // raocp_cp_batch_aa_log: the log holds every instance's last solve
    bt.a_log_rows = rows;
    return RAOCP_OK;
}

// the same loop on the host for a context k_cpb does not cover: per step the running instances'
// solves through batch_run_seq, the plant step and the stage cost in host arithmetic
int batch_mpc_seq(raocp_ctx* c, int B, int T, const double* x0, const int* scen, int max_iters, double tol,
                  double alpha, int warm, double* X, double* U, double* cost, int* status, int* iters, double* err) {
    auto& bt = c->bt;
    const int nx = c->nx, nu = c->nu;
    const size_t P = (size_t)c->P, D = (size_t)c->D, rows = (size_t)max_iters + 1;
    if (c->h_mpc_ab.empty()) return fail(RAOCP_ERR_STATE, "no plant tables for the root's children");
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    std::vector<double> xc(x0, x0 + (size_t)B * nx), Z((size_t)B * P, 0.0), E((size_t)B * D, 0.0), U0((size_t)B * nu, 0.0);
    std::vector<int> frz(B, -1), act, st(B), itv(B);
    std::vector<double> ax, az, ae, eh((size_t)B * rows * 3), dh((size_t)B * rows * 3);
    std::vector<double> xs(xc);  // the state each instance's last solve was solved from
    for (int b = 0; b < B; ++b) std::copy(x0 + (size_t)b * nx, x0 + (size_t)(b + 1) * nx, X + (size_t)b * (T + 1) * nx);
    auto blank = [&](int b, int t) {
        const size_t bt_ = (size_t)b * T + t;
        for (int r = 0; r < nx; ++r) X[((size_t)b * (T + 1) + t + 1) * nx + r] = qnan;
        for (int r = 0; r < nu; ++r) U[bt_ * nu + r] = qnan;
        cost[bt_] = qnan;
        status[bt_] = 2;
    };
    for (int t = 0; t < T; ++t) {
        act.clear();
        for (int b = 0; b < B; ++b) {
            if (frz[b] < 0) {
                act.push_back(b);
                continue;
            }
            blank(b, t);
            iters[(size_t)b * T + t] = 0;
            for (int q = 0; q < 3; ++q) err[((size_t)b * T + t) * 3 + q] = qnan;
        }
        if (act.empty()) continue;
        const int nA = (int)act.size();
        const bool cont = warm && t > 0;
        ax.resize((size_t)nA * nx);
        for (int q = 0; q < nA; ++q) std::copy(xc.begin() + (size_t)act[q] * nx, xc.begin() + (size_t)(act[q] + 1) * nx, ax.begin() + (size_t)q * nx);
        if (cont) {
            az.resize((size_t)nA * P);
            ae.resize((size_t)nA * D);
            for (int q = 0; q < nA; ++q) {
                std::copy(Z.begin() + act[q] * P, Z.begin() + (act[q] + 1) * P, az.begin() + q * P);
                std::copy(E.begin() + act[q] * D, E.begin() + (act[q] + 1) * D, ae.begin() + q * D);
            }
        }
        const int rc = batch_run_seq(c, nA, ax.data(), cont ? az.data() : nullptr, cont ? ae.data() : nullptr, max_iters, tol,
                                     alpha, st.data(), itv.data(), eh.data(), dh.data());
        bt.B = 0;
        if (rc) return rc;
        for (int q = 0; q < nA; ++q) {
            const int b = act[q];
            const size_t bt_ = (size_t)b * T + t;
            std::copy(xc.begin() + (size_t)b * nx, xc.begin() + (size_t)(b + 1) * nx, xs.begin() + (size_t)b * nx);
            std::copy(bt.hz.begin() + q * P, bt.hz.begin() + (q + 1) * P, Z.begin() + b * P);
            std::copy(bt.he.begin() + q * D, bt.he.begin() + (q + 1) * D, E.begin() + b * D);
            std::copy(bt.hu0.begin() + (size_t)q * nu, bt.hu0.begin() + (size_t)(q + 1) * nu, U0.begin() + (size_t)b * nu);
            iters[bt_] = itv[q];
            for (int r = 0; r < 3; ++r) err[bt_ * 3 + r] = itv[q] > 0 ? eh[((size_t)q * rows + itv[q] - 1) * 3 + r] : qnan;
            if (st[q] == 2) {
                frz[b] = t;
                blank(b, t);
                continue;
            }
            status[bt_] = st[q];
            const int j = scen[bt_];
            const double* A = c->h_mpc_ab.data() + (size_t)j * (nx + nu) * nx;
            const double* Bm = A + (size_t)nx * nx;
            const double* SQ = c->h_mpc_w.data() + (size_t)j * ((size_t)nx * nx + (size_t)nu * nu);
            const double* SR = SQ + (size_t)nx * nx;
            const double* x = xc.data() + (size_t)b * nx;
            const double* u = U0.data() + (size_t)b * nu;
            double* xp = X + ((size_t)b * (T + 1) + t + 1) * nx;
            double l = 0.0;
            for (int r = 0; r < nx; ++r) {
                double s = 0.0, w = 0.0;
                for (int k = 0; k < nx; ++k) s = std::fma(A[(size_t)r * nx + k], x[k], s);
                for (int k = 0; k < nu; ++k) s = std::fma(Bm[(size_t)r * nu + k], u[k], s);
                for (int k = 0; k < nx; ++k) w = std::fma(SQ[(size_t)r * nx + k], x[k], w);
                xp[r] = s;
                l += w * w;
            }
            for (int r = 0; r < nu; ++r) {
                double w = 0.0;
                for (int k = 0; k < nu; ++k) w = std::fma(SR[(size_t)r * nu + k], u[k], w);
                l += w * w;
                U[bt_ * nu + r] = u[r];
            }
            cost[bt_] = l;
            std::copy(xp, xp + nx, xc.begin() + (size_t)b * nx);
        }
    }
    bt.hz = Z;
    bt.he = E;
    bt.hu0 = U0;
    bt.hx0 = xs;
    mpc_final_k(bt.fk, B, T, iters);
    bt.B = B;
    bt.kernel = false;
    return RAOCP_OK;
}

}  // namespace

extern "C" {

int raocp_evaluate(raocp_ctx* c, const double* z, int flags, double* out, double* node_values) {
    DevGuard dg_(c);
    SweepLock sl_(c);
    if (!c || !out) return fail(RAOCP_ERR_ARG, "null argument");
    if (c->comm || c->sh_R != 1) return fail(RAOCP_ERR_STATE, "the evaluation is not available on a sharded context");
    if (!c->has_x0) return fail(RAOCP_ERR_STATE, "no initial state has been set");
    int rc;
    if ((rc = eval_ensure(c))) return rc;
    const void* dz = c->cur_z;
    if (z && (flags & RAOCP_DEVICE_PTR)) {
        dz = z;
    } else if (z) {
        if ((rc = copy_in(c, c->tmpP, z, (size_t)c->P, 0))) return rc;
        dz = c->tmpP;
    }
    return eval_run(c, dz, c->x0, out, node_values);
}

int raocp_cp_batch_evaluate(raocp_ctx* c, double* out) {
    DevGuard dg_(c);
    SweepLock sl_(c);
    if (!c || !out) return fail(RAOCP_ERR_ARG, "null argument");
    if (c->comm || c->sh_R != 1) return fail(RAOCP_ERR_STATE, "the evaluation is not available on a sharded context");
    if (c->bt.B < 1) return fail(RAOCP_ERR_STATE, "no batch has been run");
    return c->bt.kernel ? batch_eval_kernel(c, out) : batch_eval_seq(c, out);
}

int raocp_cp_batch_run(raocp_ctx* c, int B, const double* x0, const double* z0, const double* eta0, int max_iters,
                       double tol, double alpha, int* status, int* iters, double* err_hist, double* delta_hist) {
    return batch_run(c, B, x0, z0, eta0, max_iters, tol, alpha, status, iters, err_hist, delta_hist, nullptr);
}

int raocp_cp_batch_run_aa(raocp_ctx* c, int B, const double* x0, const double* z0, const double* eta0, int max_iters,
                          double tol, double alpha, int accel, int accel_every, double accel_reg, double accel_safeguard,
                          int* status, int* iters, double* err_hist, double* delta_hist) {
    const AaOpt aa{accel, accel_every, accel_reg, accel_safeguard};
    return batch_run(c, B, x0, z0, eta0, max_iters, tol, alpha, status, iters, err_hist, delta_hist, &aa);
}

int raocp_cp_batch_aa_log(raocp_ctx* c, int b, double* out) {
    DevGuard dg_(c);
    if (!c || !out) return fail(RAOCP_ERR_ARG, "null argument");
    const auto& bt = c->bt;
    if (bt.B < 1 || !bt.accel) return fail(RAOCP_ERR_STATE, "no accelerated batch has been run");
    if (b < 0 || b >= bt.B) return fail(RAOCP_ERR_ARG, "instance index out of range");
    const size_t n = (size_t)(bt.fk[b] + 1) * raocp::kAaRec;
    HIPCHK(hipMemcpy(out, bt.alog + (size_t)b * bt.a_log_rows * raocp::kAaRec, n * sizeof(double), hipMemcpyDeviceToHost));
    return RAOCP_OK;
}

int raocp_cp_batch_get(raocp_ctx* c, int b, double* z, double* eta) { return batch_get(c, b, z, eta, false); }

int raocp_cp_batch_get_prev(raocp_ctx* c, int b, double* z, double* eta) { return batch_get(c, b, z, eta, true); }

int raocp_cp_batch_first_inputs(raocp_ctx* c, double* u0) {
    DevGuard dg_(c);
    if (!c || !u0) return fail(RAOCP_ERR_ARG, "null argument");
    const auto& bt = c->bt;
    if (bt.B < 1) return fail(RAOCP_ERR_STATE, "no batch has been run");
    if (!bt.kernel) {
        std::copy(bt.hu0.begin(), bt.hu0.end(), u0);
        return RAOCP_OK;
    }
    HIPCHK(hipMemcpy(u0, bt.u0, (size_t)bt.B * c->nu * sizeof(double), hipMemcpyDeviceToHost));
    return RAOCP_OK;
}

}  // extern "C"

namespace {

// raocp_cp_batch_mpc (aa == nullptr) and raocp_cp_batch_mpc_aa: the checks of the plain call in the
// order it has always made them, then those of an accelerated call, then the loop
int batch_mpc(raocp_ctx* c, int B, int T, const double* x0, const int* scen, int max_iters, double tol, double alpha,
              int warm, double* X, double* U, double* cost, int* status, int* iters, double* err, const AaOpt* aa,
              int* aa_counts) {
    DevGuard dg_(c);
    if (!c || !x0 || !scen || !X || !U || !cost || !status || !iters || !err || (aa && !aa_counts))
        return fail(RAOCP_ERR_ARG, "null argument");
    if (B < 1 || B > 4096) return fail(RAOCP_ERR_ARG, "batch size must be in 1 .. 4096");
    if (T < 1) return fail(RAOCP_ERR_ARG, "the number of steps must be >= 1");
    if (max_iters < 0) return fail(RAOCP_ERR_ARG, "max_iters must be >= 0");
    if (c->comm || c->sh_R != 1) return fail(RAOCP_ERR_STATE, "batched solves are not available on a sharded context");
    const int nc = c->h_nch.empty() ? 0 : c->h_nch[0];
    for (size_t q = 0; q < (size_t)B * T; ++q)
        if (scen[q] < 0 || scen[q] >= nc)
            return fail(RAOCP_ERR_ARG, "scenario entry " + std::to_string(scen[q]) + " is not a child of the root (0 .. " +
                                           std::to_string(nc - 1) + ")");
    int rc;
    if (aa && ((rc = aa_check_opt(*aa)) || (rc = aa_check_ctx(c)))) return rc;
    c->bt.B = 0;
    c->bt.accel = false;
    if (aa || cpb_on(c))
        return batch_mpc_kernel(c, B, T, x0, scen, max_iters, tol, alpha, warm, X, U, cost, status, iters, err, aa, aa_counts);
    return batch_mpc_seq(c, B, T, x0, scen, max_iters, tol, alpha, warm, X, U, cost, status, iters, err);
}

}  // namespace

extern "C" {

int raocp_cp_batch_mpc(raocp_ctx* c, int B, int T, const double* x0, const int* scen, int max_iters, double tol,
                       double alpha, int warm, double* X, double* U, double* cost, int* status, int* iters, double* err) {
    return batch_mpc(c, B, T, x0, scen, max_iters, tol, alpha, warm, X, U, cost, status, iters, err, nullptr, nullptr);
}

int raocp_cp_batch_mpc_aa(raocp_ctx* c, int B, int T, const double* x0, const int* scen, int max_iters, double tol,
                          double alpha, int warm, int accel, int accel_every, double accel_reg, double accel_safeguard,
                          double* X, double* U, double* cost, int* status, int* iters, double* err, int* aa_counts) {
    const AaOpt aa{accel, accel_every, accel_reg, accel_safeguard};
    return batch_mpc(c, B, T, x0, scen, max_iters, tol, alpha, warm, X, U, cost, status, iters, err, &aa, aa_counts);
}

}  // extern "C"
