// raocp_capi.hip — host side of libraocp_hip.so: the C-ABI declared in
// include/raocp_hip.h, except the batched solves, the closed-loop simulation and the
// evaluation (raocp_batch.hip, host code only). Owns one HIP device context per raocp_ctx:
// uploads the packed problem, keeps the CP iterate resident in HBM, launches the kernels of
// raocp_kernels.hip and replays the CP iteration as a captured hipGraph. What the two host
// units share is in raocp_host.h.

#include "raocp_kernels.hip"
#include "raocp_dynr.h"
#include "raocp_drxfer.h"
#include "raocp_cp4.h"
#include "raocp_cp5.h"
#include "raocp_cpb.h"
#include "raocp_eval.h"
#include "../../include/raocp_hip.h"

#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <random>
#include <string>
#include <vector>

#include "raocp_host.h"

using raocp::kBlock;

// host fp64 arrays <-> the context's device vectors (fp32 contexts convert on the host;
// a device pointer is taken in the context's own type)
int raocp::copy_in(raocp_ctx* c, double* dst, const double* src, size_t count, int flags) {
    if (c->f32 && !(flags & RAOCP_DEVICE_PTR)) {
        std::vector<float> tmp(src, src + count);
        HIPCHK(hipMemcpyAsync(dst, tmp.data(), count * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return RAOCP_OK;
    }
    HIPCHK(hipMemcpyAsync(dst, src, count * c->wsz,
                          (flags & RAOCP_DEVICE_PTR) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    return RAOCP_OK;
}

int raocp::copy_out(raocp_ctx* c, double* dst, const double* src, size_t count, int flags) {
    if (c->f32 && !(flags & RAOCP_DEVICE_PTR)) {
        std::vector<float> tmp(count);
        HIPCHK(hipMemcpyAsync(tmp.data(), src, count * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        std::copy(tmp.begin(), tmp.end(), dst);
        return RAOCP_OK;
    }
    HIPCHK(hipMemcpyAsync(dst, src, count * c->wsz,
                          (flags & RAOCP_DEVICE_PTR) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
    if (!(flags & RAOCP_DEVICE_PTR)) HIPCHK(hipStreamSynchronize(c->stream));
    return RAOCP_OK;
}

// a table as the context's scalar type (fp32 contexts keep float arrays in the Dev's
// double* fields; only the T-templated kernels read them)
int raocp::upload_t(raocp_ctx* c, const double** dst, const std::vector<double>& v) {
    if (!c->f32) return c->upload_vec(dst, v);
    std::vector<float> f(v.begin(), v.end());
    const float* p = nullptr;
    int rc = c->upload_vec(&p, f);
    *dst = (const double*)p;
    return rc;
}

namespace {

// row-major table [cnt][rows][cols] -> column-major per matrix: out[k*rows + r] = M[r][k]
std::vector<double> to_colmajor(const double* src, int cnt, int rows, int cols) {
    std::vector<double> out((size_t)cnt * rows * cols);
    for (int t = 0; t < cnt; ++t)
        for (int r = 0; r < rows; ++r)
            for (int k = 0; k < cols; ++k)
                out[(size_t)t * rows * cols + (size_t)k * rows + r] = src[(size_t)t * rows * cols + (size_t)r * cols + k];
    return out;
}

std::vector<double> copy_table(const double* src, size_t count) {
    return std::vector<double>(src, src + count);
}

struct Launch {
    int G, per, blocks;
};

Launch groups(int G, int count) {
    Launch l;
    l.G = G;
    l.per = kBlock / G;
    l.blocks = cdiv(count, l.per);
    return l;
}

int check_group(int G, const char* what) {
    if (G > kBlock)
        return fail(RAOCP_ERR_ARG, std::string("group size of ") + what + " (" + std::to_string(G) +
                                       ") exceeds the 256-lane workgroup; nx/nu/children too large for this build");
    return RAOCP_OK;
}

// ---- template dispatch on (nx, nu): exact sizes get fully unrolled kernels,
// everything else runs the runtime-size instantiation <0, 0>.
template <class F, class... A>
void dispatch(int nx, int nu, F f, A... a) {
    if (nx == 20 && nu == 8) f.template run<20, 8>(a...);
    else if (nx == 32 && nu == 12) f.template run<32, 12>(a...);
    else if (nx == 64 && nu == 16) f.template run<64, 16>(a...);
    else if (nx == 3 && nu == 2) f.template run<3, 2>(a...);
    else f.template run<0, 0>(a...);
}

// the MFMA CP kernels are instantiated per (row tiles of nx, row tiles of nu)
template <class F, class... A>
void dispatch_rt(int nx, int nu, F f, A... a) {
    const int rx = (nx + 15) / 16, ru = (nu + 15) / 16;
    if (ru == 1) {
        if (rx == 1) f.template run<1, 1>(a...);
        else if (rx == 2) f.template run<2, 1>(a...);
        else if (rx == 3) f.template run<3, 1>(a...);
        else f.template run<4, 1>(a...);
    } else {
        if (rx == 1) f.template run<1, 2>(a...);
        else if (rx == 2) f.template run<2, 2>(a...);
        else if (rx == 3) f.template run<3, 2>(a...);
        else f.template run<4, 2>(a...);
    }
}
template <class K>
void allow_lds(K kernel, size_t bytes) {
    if (bytes > 64 * 1024) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                      (int)bytes);
}

// ---- launches (all on c->stream)
struct EllOp {
    template <int NX, int NU>
    void run(raocp_ctx* c, const double* z, double* eta) {
        auto k = raocp::k_ell<NX, NU>;
        allow_lds(k, c->ell_lds);
        if (c->ell_nb) k<<<c->ell_nb, c->ell_threads, c->ell_lds, c->stream>>>(c->dev, z, eta);
    }
};
template <class T>
struct Ell2Op {
    template <int RX, int RU>
    void run(raocp_ctx* c, const double* z, double* eta, bool t) {
        if (t) {
            auto k = raocp::k_ellt2<T, RX, RU>;
            allow_lds(k, c->lds_cpp2);
            k<<<c->cp2_nbF + c->cp2_nbL, 64 * c->cp2_W, c->lds_cpp2, c->stream>>>(c->dev, z, eta, c->cp2_nbF);
        } else {
            auto k = raocp::k_ell2<T, RX, RU>;
            allow_lds(k, c->lds_cpd2);
            k<<<c->cp2_nbF + c->cp2_nbL, 64 * c->cp2_W, c->lds_cpd2, c->stream>>>(c->dev, z, eta, c->cp2_nbF);
        }
    }
};
// L as streaming wave tasks (raocp_ell3.hip): compile-time sizes of the benchmark configs
template <class T>
bool launch_ell3(raocp_ctx* c, const double* z, double* eta) {
    const int g = c->ell3_grid;
    if (c->nx == 20 && c->nu == 8) raocp::k_ell3<T, 20, 8><<<g, 256, 0, c->stream>>>(c->dev, z, eta, c->unif_C, c->box_mode);
    else if (c->nx == 32 && c->nu == 12) raocp::k_ell3<T, 32, 12><<<g, 256, 0, c->stream>>>(c->dev, z, eta, c->unif_C, c->box_mode);
    else if (c->nx == 64 && c->nu == 16) raocp::k_ell3<T, 64, 16><<<g, 256, 0, c->stream>>>(c->dev, z, eta, c->unif_C, c->box_mode);
    else return false;
    return true;
}
// k_ell2 / k_ellt2 hold one sqrtQ, sqrtR and sqrtPf fragment per node block; a block whose nodes use
// different tables (a cost per mode) has no table index, so an fp32 context refuses L / L^T there
// (its CP loop runs k_cpd / k_cpp<float>, which read a table per child)
int ell_available(const raocp_ctx* c) {
    if (c->f32 && c->ell2_mixed)
        return fail(RAOCP_ERR_ARG, "fp32 L / L^T need one weight table per node block (this problem has a cost per mode); "
                                   "the CP loop is available, with a step size from an fp64 context");
    return RAOCP_OK;
}
void launch_ell(raocp_ctx* c, const double* z, double* eta) {
    if (c->ell3 && (c->f32 ? launch_ell3<float>(c, z, eta) : launch_ell3<double>(c, z, eta))) return;
    if (c->f32) dispatch_rt(c->nx, c->nu, Ell2Op<float>{}, c, z, eta, false);
    else dispatch(c->nx, c->nu, EllOp{}, c, z, eta);
}

struct EllTOp {
    template <int NX, int NU>
    void run(raocp_ctx* c, const double* eta, double* z) {
        auto k = raocp::k_ell_t<NX, NU>;
        allow_lds(k, c->ellt_lds);
        if (c->ell_nb) k<<<c->ell_nb, c->ell_threads, c->ellt_lds, c->stream>>>(c->dev, eta, z);
    }
};
// L^T as streaming wave tasks (raocp_ell3.hip): uniform tables and branching
template <class T, int QM>
bool launch_ellt3q(raocp_ctx* c, const double* eta, double* z) {
    const int g = c->ellt3_grid, C = c->ellt3_C;
    if (c->nx == 20 && c->nu == 8) raocp::k_ellt3<T, 20, 8, QM><<<g, 256, 0, c->stream>>>(c->dev, eta, z, C, c->box_mode);
    else if (c->nx == 32 && c->nu == 12) raocp::k_ellt3<T, 32, 12, QM><<<g, 256, 0, c->stream>>>(c->dev, eta, z, C, c->box_mode);
    else if (c->nx == 64 && c->nu == 16) raocp::k_ellt3<T, 64, 16, QM><<<g, 256, 0, c->stream>>>(c->dev, eta, z, C, c->box_mode);
    else return false;
    return true;
}
template <class T>
bool launch_ellt3(raocp_ctx* c, const double* eta, double* z) {
    const int C = c->ellt3_C;
    if (C == 1) return launch_ellt3q<T, 4>(c, eta, z);
    if (C == 2) return launch_ellt3q<T, 2>(c, eta, z);
    return launch_ellt3q<T, 1>(c, eta, z);
}
void launch_ell_t(raocp_ctx* c, const double* eta, double* z) {
    if (c->ellt3_C && (c->f32 ? launch_ellt3<float>(c, eta, z) : launch_ellt3<double>(c, eta, z))) return;
    if (c->f32) dispatch_rt(c->nx, c->nu, Ell2Op<float>{}, c, eta, z, true);
    else dispatch(c->nx, c->nu, EllTOp{}, c, eta, z);
}

// ---- per-stage MFMA dynamics (raocp_dyn2.hip) on z = the iterate to project
template <class T>
struct Dyn2Op {
    template <int RX, int RU>
    void run(raocp_ctx* c, double* z, const Ctl* ctl) {
        const int N = c->N, nthr = 256, W = nthr / 64;
        auto grid = [&](int nt) { return std::max(1, cdiv(nt, W)); };
        for (int t = N - 1; t >= 0; --t) {
            const int* o = &c->d2_off[(size_t)t * 5];
            const bool leaf = t + 1 == N;
            if (o[1] > o[0])
                raocp::k_d2_prod<T, RX + RU, 4 * RX><<<grid(o[1] - o[0]), nthr, 0, c->stream>>>(
                    c->dev, ctl, c->d2_tiles + o[0], o[1] - o[0], c->d2_idx, c->W2, leaf ? z : c->Q2,
                    leaf ? c->dev.X0 : 0, leaf ? T(-1) : T(1), c->PA2);
            if (o[2] > o[1])
                raocp::k_d2_node<T, RX + RU, 4 * RU><<<grid(o[2] - o[1]), nthr, 0, c->stream>>>(
                    c->dev, ctl, c->d2_tiles + o[1], o[2] - o[1], c->d2_idx, c->RG2, z, c->PA2, c->Q2, c->Dd2);
        }
        raocp::k_d2_x0<T><<<1, 64, 0, c->stream>>>(ctl, z, c->dev.X0, c->x0, c->nx);
        for (int t = 0; t < N; ++t) {
            const int* o = &c->d2_off[(size_t)t * 5];
            if (o[3] > o[2])
                raocp::k_d2_fwd<T, RU, 4 * RX, false><<<grid(o[3] - o[2]), nthr, 0, c->stream>>>(
                    c->dev, ctl, c->d2_tiles + o[2], o[3] - o[2], c->d2_idx, c->KM2, z, c->Dd2);
            if (o[4] > o[3])
                raocp::k_d2_fwd<T, RX, 4 * (RX + RU), true><<<grid(o[4] - o[3]), nthr, 0, c->stream>>>(
                    c->dev, ctl, c->d2_tiles + o[3], o[4] - o[3], c->d2_idx, c->F2, z, c->Dd2);
        }
    }
};

// the per-stage streaming sweep (raocp_dyn3.hip) on z; ck: the previous iteration's stopping
// test in an extra workgroup of the first launch (defer_check)
// part: 0 the whole projection; 1 (a shard) the backward stages below its cut, on its owned
// parents; 2 the replicated top backward, then every forward stage (owned below the cut)
// the stages k_dy3_top_back / k_dy3_top_fwd run in one workgroup: a shard merges only stages of
// its replicated top (t < sh_S, run after X2), at least two of them
int dyn3_top_stages(const raocp_ctx* c) {
    if (c->sh_S == 0) return c->d3ts;
    const int ts = std::min(c->d3ts, c->sh_S);
    return ts >= 2 ? ts : 0;
}
template <class T, int NX, int NU>
void launch_dyn3t(raocp_ctx* c, double* z, const Ctl* ctl, const raocp::ChkArg* ck, int part) {
    typedef raocp::Dy3Lds<T, NX, NU> L;
    const int C = c->unif_branch;
    constexpr int RX = (NX + 15) / 16, RU = (NU + 15) / 16;
    // LDS: the stage's tables; the backward kernel's slot sums of a cooperative tile after them
    const size_t lb = (size_t)(L::back_n(C) + C * (RU + RX) * 4 * 64) * sizeof(T), lf = (size_t)L::fwd_n(C) * sizeof(T);
    const size_t lmax = std::max(lb, lf);
    const int thr = lmax > 64 * 1024 ? 512 : 256, wpb = thr / 64;
    // (1,024-lane workgroups for the wide stages when the tables allow one workgroup per CU
    // measured slower at config 5: 215.3 vs 190.9 us per projection, profiles/r03_v3)
    // the wide stages (a wave per tile, looping) in 256-lane workgroups: at config 5 (one
    // workgroup per CU by LDS) 4 waves of 4 tiles each beat 8 waves of 2 (projection 197.1 ->
    // 191.9 us); at least 2 tiles per wave measured slower at configs 4 and 5 (fewer waves in
    // flight: 113.6 -> 123.1, 197.1 -> 217.9 us; profiles/r05/dy3_geometry.log)
    const int thr_w = 256, wpb_w = thr_w / 64;
    const int per_cu = std::max<int>(1, std::min<int>(2048 / thr_w, (int)(160 * 1024 / lmax)));
    const int cap = 256 * per_cu;  // one round of resident workgroups; waves loop over tiles
    auto kb = raocp::k_dy3_back<T, NX, NU>;
    auto kf = raocp::k_dy3_fwd<T, NX, NU>;
    allow_lds(kb, lb);
    allow_lds(kf, lf);
    // stages of few tiles run slot-parallel (a wave per child slot): the dependent MFMA chain
    // of a tile is what a small stage costs. Decided on the whole stage, so a shard sums a
    // parent's child slots in the same order as the unsharded sweep (bit-identical results).
    // (every stage slot-parallel, a workgroup looping over its tiles, measured slower: config 4
    // 112.3 vs 110.4 us, config 5 227.5 vs 197.3 us per projection, profiles/r04/cp3_time_dy3.log)
    auto coop = [&](int t) { return (c->d3st[t].i1 - c->d3st[t].i0 + 15) / 16 * C <= 256 * wpb; };
    auto grid = [&](const raocp::Dy3Stage& st, int t, bool back) {
        const int tiles = (st.i1 - st.i0 + 15) / 16;
        if (coop(t)) return std::max(1, std::min(cap, back ? tiles : (tiles * C + wpb - 1) / wpb));
        return std::max(1, std::min(cap, (tiles + wpb_w - 1) / wpb_w));
    };
    auto threads = [&](int t) { return coop(t) ? thr : thr_w; };
    const int N = c->N, S = c->sh_S;  // S > 0: a shard owns the stages >= S partly
    auto stage = [&](int t) -> const raocp::Dy3Stage& { return S > 0 && t >= S ? c->d3own[t] : c->d3st[t]; };
    // the top stages t < ts in one workgroup per direction (dyn3_top_stages)
    const int ts = dyn3_top_stages(c);
    raocp::Dy3Top tp{};
    tp.ts = ts;
    for (int t = 0; t < ts; ++t) tp.st[t] = c->d3st[t];
    tp.same_kinds = 1;
    for (int t = 1; t < ts; ++t)
        for (int k = 0; k < C; ++k) tp.same_kinds &= c->d3st[t].kind[k] == c->d3st[0].kind[k];
    const size_t ltop = (size_t)(L::back_n(C) + (8 / C) * C * (RU + RX) * 4 * 64) * sizeof(T);
    auto ktb = raocp::k_dy3_top_back<T, NX, NU>;
    auto ktf = raocp::k_dy3_top_fwd<T, NX, NU>;
    if (ts) {
        allow_lds(ktb, ltop);
        allow_lds(ktf, lf);
    }
    for (int t = N - 1; t >= ts; --t) {
        if (part == 1 && t < S) break;
        if (part == 2 && t >= S) continue;
        const raocp::Dy3Stage& st = stage(t);
        if (st.i1 <= st.i0) continue;
        raocp::ChkArg ca{};
        if (ck && t == N - 1) ca = *ck;
        const double* img = (const double*)((const char*)c->d3img_b + (size_t)t * L::back_n(C) * sizeof(T));
        kb<<<grid(st, t, true) + ca.on, threads(t), lb, c->stream>>>(c->dev, ctl, ca, z, c->Q2, c->Dd2, st, C, img,
                                                                    coop(t) ? 1 : 0);
    }
    if (part == 1) return;
    if (ts) {
        ktb<<<1, 512, ltop, c->stream>>>(c->dev, ctl, z, c->Q2, c->Dd2, tp, C, (const double*)c->d3img_b);
        ktf<<<1, 512, lf, c->stream>>>(c->dev, ctl, z, c->Dd2, c->x0, tp, C, (const double*)c->d3img_f);
    }
    for (int t = ts; t < N; ++t) {
        const raocp::Dy3Stage& st = stage(t);
        if (st.i1 <= st.i0) continue;
        const double* img = (const double*)((const char*)c->d3img_f + (size_t)t * L::fwd_n(C) * sizeof(T));
        kf<<<grid(st, t, false), threads(t), lf, c->stream>>>(c->dev, ctl, z, c->Dd2, c->x0, st, C, img,
                                                               coop(t) ? 1 : 0);
    }
}
// LDS bytes of the sweep's larger launch (tables + the slot-parallel sums; launch_dyn3t)
template <class T, int NX, int NU>
size_t dyn3_lds(int C) {
    typedef raocp::Dy3Lds<T, NX, NU> L;
    constexpr int RX = (NX + 15) / 16, RU = (NU + 15) / 16;
    return std::max((size_t)(L::back_n(C) + C * (RU + RX) * 4 * 64) * sizeof(T), (size_t)L::fwd_n(C) * sizeof(T));
}
bool dyn3_lds_fits(bool f32, int nx, int nu, int C) {
    size_t b = ~(size_t)0;
    if (nx == 20 && nu == 8) b = f32 ? dyn3_lds<float, 20, 8>(C) : dyn3_lds<double, 20, 8>(C);
    else if (nx == 32 && nu == 12) b = f32 ? dyn3_lds<float, 32, 12>(C) : dyn3_lds<double, 32, 12>(C);
    else if (nx == 64 && nu == 16 && f32) b = dyn3_lds<float, 64, 16>(C);
    // (fp64 at nx = 64: the tables exceed the LDS, so k_dy3 has no such instantiation)
    return b <= 160 * 1024;
}
// the per-stage table images of the sweep, laid out once (k_dy3_image, one workgroup per stage)
template <class T, int NX, int NU>
int dyn3_imagest(raocp_ctx* c) {
    typedef raocp::Dy3Lds<T, NX, NU> L;
    const int C = c->unif_branch, N = (int)c->d3st.size();
    const size_t nb = (size_t)L::back_n(C) * sizeof(T) / 8, nf = (size_t)L::fwd_n(C) * sizeof(T) / 8;
    c->d3nb = nb;
    c->d3nf = nf;
    int rc;
    if ((rc = c->alloc(&c->d3img_b, std::max<size_t>(1, N * nb))) || (rc = c->alloc(&c->d3img_f, std::max<size_t>(1, N * nf))))
        return rc;
    // the top stages of at most two rounds of 512 / (64 C) tiles run in one workgroup per
    // direction (k_dy3_top_back / k_dy3_top_fwd); RAOCP_DY3_TOP=0 keeps a launch per stage
    {
        constexpr int RX = (NX + 15) / 16, RU = (NU + 15) / 16;
        const int tpr = 8 / C;
        const size_t ltop = (size_t)(L::back_n(C) + tpr * C * (RU + RX) * 4 * 64) * sizeof(T);
        // (stages of up to 4 / 16 rounds measured slower: config 4 117.8 / 145.4 vs 111.6 us,
        // profiles/r04/cp3_time_dy3_rounds.log)
        const int rounds = 2;
        int ts = 0;
        while (ts < N - 1 && ts < raocp::kDy3TopMax && (c->d3st[ts].i1 - c->d3st[ts].i0 + 15) / 16 <= rounds * tpr) ++ts;
        if (ts < 2 || ltop > 159 * 1024 || (size_t)L::fwd_n(C) * sizeof(T) > 159 * 1024) ts = 0;
        if (!env_flag("RAOCP_DY3_TOP", true)) ts = 0;
        c->d3ts = ts;
    }
    for (int t = 0; t < N; ++t)
        raocp::k_dy3_image<T, NX, NU><<<1, 512, 0, c->stream>>>(c->d3st[t], C, c->W2, c->RG2, c->KM2, c->F2,
                                                                c->d3img_b + t * nb, c->d3img_f + t * nf);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return RAOCP_OK;
}
int dyn3_images(raocp_ctx* c) {
    if (c->f32) {
        if (c->nx == 20) return dyn3_imagest<float, 20, 8>(c);
        if (c->nx == 32) return dyn3_imagest<float, 32, 12>(c);
        return dyn3_imagest<float, 64, 16>(c);
    }
    if (c->nx == 20) return dyn3_imagest<double, 20, 8>(c);
    if (c->nx == 32) return dyn3_imagest<double, 32, 12>(c);
    return fail(RAOCP_ERR_ARG, "k_dy3 has no fp64 form at nx = 64 (dyn3_lds_fits)");
}
void launch_dyn3(raocp_ctx* c, double* z, const Ctl* ctl, const raocp::ChkArg* ck, int part) {
    if (c->f32) {
        if (c->nx == 20) launch_dyn3t<float, 20, 8>(c, z, ctl, ck, part);
        else if (c->nx == 32) launch_dyn3t<float, 32, 12>(c, z, ctl, ck, part);
        else launch_dyn3t<float, 64, 16>(c, z, ctl, ck, part);
    } else {
        // (no fp64 nx = 64 form: dyn3_lds_fits keeps such contexts off k_dy3)
        if (c->nx == 20) launch_dyn3t<double, 20, 8>(c, z, ctl, ck, part);
        else if (c->nx == 32) launch_dyn3t<double, 32, 12>(c, z, ctl, ck, part);
    }
}

// workgroups per CU of the split sweep's two kernels at their LDS sizes (co-residency)
struct SplitOcc {
    template <int NX, int NU>
    void run(raocp_ctx* c, int* pu, int* pd) {
        auto ku = raocp::k_dyn_up<NX, NU>;
        auto kd = c->f_lds_top ? raocp::k_dyn_down<NX, NU, true> : raocp::k_dyn_down<NX, NU, false>;
        allow_lds(ku, c->lds_up);
        allow_lds(kd, c->lds_down);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(pu, (const void*)ku, raocp::kFuseBlock, c->lds_up) != hipSuccess)
            *pu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(pd, (const void*)kd, raocp::kFuseBlock, c->lds_down) != hipSuccess)
            *pd = 0;
    }
};

struct DynOp {
    // part: 0 whole projection; 1 the tiers' backward sweeps only; 2 the top and the
    // tiers' forward sweeps (a shard exchanges the roots' q rows in between)
    template <int NX, int NU>
    void run(raocp_ctx* c, raocp::Bufs bf, int zsel, const Ctl* ctl, int part, const raocp::ChkArg* ck) {
        const int s = c->cut;
        const int B = c->dyn_block;
        // diagnostics: each launch stamps into its own 64-slot region
        Dev dv = c->dev;
        int slot = 0;
        auto dev_for = [&]() {
            if (c->dev.stamps) dv.stamps = c->dev.stamps + 64 * slot++;
            return dv;
        };
        const bool sharded = c->sh_S > 0;
        auto tier_arg = [&](int k) {  // a shard launches only the subtrees it owns
            raocp::TierArg ta = c->tiers[k].ta;
            ta.boff = sharded ? c->tier_own[k].first : 0;
            return ta;
        };
        auto tier_blocks = [&](int k) { return sharded ? c->tier_own[k].second : c->tiers[k].nsub; };
        if (c->path.dyn == DynPath::TiersSplit) {
            // the tiered sweep in two launches (raocp_dynf.hip): one workgroup per subtree of
            // every tier plus the top; k_dyn_up runs the deferred stopping test in block 0
            raocp::FuseArg fa = c->fuse;
            if (ck) fa.ck = *ck;
            int nsub = 0;
            for (const auto& tp : c->tiers) nsub += tp.nsub;
            auto ku = raocp::k_dyn_up<NX, NU>;
            auto kd = c->f_lds_top ? raocp::k_dyn_down<NX, NU, true> : raocp::k_dyn_down<NX, NU, false>;
            allow_lds(ku, c->lds_up);
            allow_lds(kd, c->lds_down);
            ku<<<nsub + 1 + (fa.ck.on ? 1 : 0), raocp::kFuseBlock, c->lds_up, c->stream>>>(dev_for(), bf, ctl, zsel, c->q,
                                                                                           c->d, fa);
            kd<<<nsub + 1, raocp::kFuseBlock, c->lds_down, c->stream>>>(dev_for(), bf, ctl, zsel, c->d, c->x0, fa);
            return;
        }
        if (c->path.dyn == DynPath::Tiers) {
            // tiers below the top, deepest first (backward), the top, then the tiers (forward)
            if (part != 2)
                for (int k = (int)c->tiers.size() - 1; k >= 0; --k) {
                    const auto& tp = c->tiers[k];
                    const int c0 = c->cls_ptr[tp.s0], c1 = c->cls_ptr[tp.s1];
                    const int p0 = c->pair_ptr[c0], p1 = c->pair_ptr[c1];
                    auto kb = tp.fold ? raocp::k_dyn_bottom_back<NX, NU, true> : raocp::k_dyn_bottom_back<NX, NU, false>;
                    allow_lds(kb, tp.lds_b);
                    // the deepest tier (launched first) carries the deferred stopping test
                    raocp::ChkArg cka{};
                    raocp::TierArg ta = tier_arg(k);
                    if (ck && k == (int)c->tiers.size() - 1) {
                        cka = *ck;
                        ta.boff -= 1;
                    }
                    if (tier_blocks(k) > 0)
                        kb<<<tier_blocks(k) + cka.on, B, tp.lds_b, c->stream>>>(dev_for(), bf, ctl, zsel, c->q, c->d, tp.s0,
                                                                               tp.s1, tp.maxch, c0, c1, p0, p1, tp.lv, ta, cka);
                }
            if (part == 1) return;
            {
                const int c1 = c->cls_ptr[s], p1 = c->pair_ptr[c1];
                auto kt = c->f_lds_top ? (c->fold_top ? raocp::k_dyn_top<NX, NU, true, true> : raocp::k_dyn_top<NX, NU, true, false>)
                                       : (c->fold_top ? raocp::k_dyn_top<NX, NU, false, true> : raocp::k_dyn_top<NX, NU, false, false>);
                allow_lds(kt, c->lds_top);
                const int T = c->stage_ptr[s], nb = c->stage_ptr[s + 1] - T;
                kt<<<1, c->dyn_top_block, c->lds_top, c->stream>>>(dev_for(), bf, ctl, zsel, c->q, c->x0, s, c->maxch_top, c1,
                                                                   p1, T, nb);
            }
            for (int k = 0; k < (int)c->tiers.size(); ++k) {
                const auto& tp = c->tiers[k];
                const int c0 = c->cls_ptr[tp.s0], c1 = c->cls_ptr[tp.s1], p0 = c->pair_ptr[c0], p1 = c->pair_ptr[c1];
                auto kf = tp.fm == 1 ? raocp::k_dyn_bottom_fwd<NX, NU, 1>
                                     : (tp.fm == 2 ? raocp::k_dyn_bottom_fwd<NX, NU, 2> : raocp::k_dyn_bottom_fwd<NX, NU, 0>);
                allow_lds(kf, tp.lds_f);
                if (tier_blocks(k) > 0)
                    kf<<<tier_blocks(k), B, tp.lds_f, c->stream>>>(dev_for(), bf, ctl, zsel, c->d, tp.s0, tp.s1, c0, c1,
                                                                  p0, p1, tp.lv, tier_arg(k));
            }
            return;
        }
        if (part == 2) return;  // the per-stage path runs whole in part 1 / 0
        // per-stage path on padded global rows
        const int R = c->nu + c->nx;
        raocp::k_dyn_gather<NX, NU><<<std::max(1, std::min(1024, cdiv(c->n * c->KP, kBlock))), kBlock, 0, c->stream>>>(
            c->dev, bf, ctl, zsel, c->gXQ, c->gU, c->gXD);
        for (int t = c->N - 1; t >= 0; --t) {
            const int b = c->stage_ptr[t], e = c->stage_ptr[t + 1];
            const int cb = e, ce = c->stage_ptr[t + 2];
            const int slots_a = B / (R * raocp::kKS), slots_b = B / R;
            raocp::k_dyn_stage_a<NX, NU><<<cdiv(ce - cb, slots_a), B, 0, c->stream>>>(
                c->dev, ctl, c->gXQ, c->gP, cb, ce, t + 1 == c->N ? -1.0 : 1.0);
            raocp::k_dyn_stage_b<NX, NU><<<cdiv(e - b, slots_b), B, 0, c->stream>>>(c->dev, ctl, c->gXQ, c->gU,
                                                                                         c->gP, c->gXD, c->d, b, e);
        }
        const int per_node = c->nu * raocp::kKS + c->cmax * c->nx * raocp::kKS;
        const int slots_f = std::max(1, B / per_node);
        for (int t = 0; t < c->N; ++t) {
            const int b = c->stage_ptr[t], e = c->stage_ptr[t + 1];
            raocp::k_dyn_stage_f<NX, NU><<<cdiv(e - b, slots_f), B, 0, c->stream>>>(c->dev, bf, ctl, zsel, c->gXD,
                                                                                         c->x0, b, e);
        }
    }
};
// dynamics projection on z = Z[(k + zsel) % 3] (k from ctl when ctl != null, else 0)
// ck: the previous CP iteration's stopping test, run by an extra workgroup of the first
// launch (only where defer_check(c) holds)
void launch_dynamics(raocp_ctx* c, raocp::Bufs bf, int zsel, const Ctl* ctl, int part = 0,
                     const raocp::ChkArg* ck = nullptr) {
    double* z = zsel % 3 == 0 ? bf.z0 : (zsel % 3 == 1 ? bf.z1 : bf.z2);
    switch (c->path.dyn) {
        case DynPath::Dr: {  // the regular-tree sweep (raocp_dynr.hip): never a shard's, so always whole
            raocp::DrPlan p = c->drp;
            if (c->dev.stamps) p.stamps = c->dev.stamps;
            raocp::dr_launch(p, c->nx, c->nu, c->dr_lds, bf, zsel, ctl,
                             ck ? *ck : raocp::ChkArg{nullptr, nullptr, nullptr, 0, 0}, c->stream);
            return;
        }
        case DynPath::Dyn3: launch_dyn3(c, z, ctl, ck, part); return;
        case DynPath::Dyn2:
            if (c->f32) dispatch_rt(c->nx, c->nu, Dyn2Op<float>{}, c, z, ctl);
            else dispatch_rt(c->nx, c->nu, Dyn2Op<double>{}, c, z, ctl);
            return;
        default: dispatch(c->nx, c->nu, DynOp{}, c, bf, zsel, ctl, part, ck); return;  // TiersSplit, Tiers, PerStage
    }
}

// the device word a hand-off sweep sets when a wait times out (nullptr: no such sweep)
const unsigned* err_word(const raocp_ctx* c) {
    if (c->path.dyn == DynPath::Dr) return c->drp.sync + 1;
    if (c->path.dyn == DynPath::TiersSplit && c->fuse_sync) return (const unsigned*)c->fuse_sync + 1;
    return nullptr;
}
// the fused sweep's error word (a hand-off wait timed out, raocp_dynf.hip): checked after
// every synchronised run that may have launched it; the context is unusable afterwards
int fuse_err(raocp_ctx* c) {
    const unsigned* w = err_word(c);
    unsigned e = 0;
    if (w) HIPCHK(hipMemcpy(&e, w, sizeof(unsigned), hipMemcpyDeviceToHost));
    if (!e) return RAOCP_OK;
    if (c->path.dyn == DynPath::Dr) {  // a clean protocol state: the epoch, the error word and every granule
        HIPCHK(hipMemset(c->drp.sync, 0, 2 * sizeof(unsigned)));
        HIPCHK(hipMemset(c->drp.gq, 0, c->dr_gran * sizeof(unsigned long long)));
        HIPCHK(hipMemset(c->drp.gx, 0, c->dr_gran * sizeof(unsigned long long)));
        return fail(RAOCP_ERR_STATE, "dynamics sweep: a workgroup hand-off timed out (k_dr); "
                                     "RAOCP_DR=0 selects the tiered sweep");
    }
    HIPCHK(hipMemset(c->fuse_sync, 0, c->fuse_words * sizeof(unsigned)));
    return fail(RAOCP_ERR_STATE, "dynamics sweep: a workgroup hand-off timed out (k_dyn_up / k_dyn_down); "
                                 "RAOCP_DYN_SPLIT=0 selects the tier launches");
}

// role: 0 all blocks; 1 nonleaf blocks only; 2 leaf blocks only (op_bench timing)
struct CpPrimalOp {
    template <int NX, int NU>
    void run(raocp_ctx* c, bool full, int role) {
        const Launch a = groups(c->nx + c->nu + c->cmax + 1, c->m);
        const Launch l = groups(c->nx, c->n - c->m);
        int grid = a.blocks + l.blocks, blk0 = 0;
        if (role == 1) grid = a.blocks;
        if (role == 2) { grid = l.blocks; blk0 = a.blocks; }
        if (full)
            raocp::k_cp_primal<true, NX, NU><<<grid, kBlock, 0, c->stream>>>(c->dev, c->ctl, c->bufs, c->XI2,
                                                                              c->redpart, a.blocks, blk0);
        else
            raocp::k_cp_primal<false, NX, NU><<<grid, kBlock, 0, c->stream>>>(c->dev, c->ctl, c->bufs, c->XI2,
                                                                               c->redpart, a.blocks, blk0);
    }
};
void launch_cp_primal(raocp_ctx* c, bool full, int role = 0) { dispatch(c->nx, c->nu, CpPrimalOp{}, c, full, role); }

// role: 0 all blocks; 1 child; 2 nonleaf; 3 leaf blocks only (op_bench timing)
struct CpDualOp {
    template <int NX, int NU>
    void run(raocp_ctx* c, bool with_l, double* dsolo, int mode, int role) {
        const Launch a = groups(c->nx + c->nu + 2, c->n - 1);
        const Launch b = groups(2 * c->cmax + 2 + c->nx + c->nu, c->m);
        const Launch l = groups(2 * c->nx + 2, c->n - c->m);
        int grid = a.blocks + b.blocks + l.blocks, blk0 = 0;
        if (role == 1) grid = a.blocks;
        if (role == 2) { grid = b.blocks; blk0 = a.blocks; }
        if (role == 3) { grid = l.blocks; blk0 = a.blocks + b.blocks; }
        if (with_l)
            raocp::k_cp_dual<true, NX, NU><<<grid, kBlock, 0, c->stream>>>(c->dev, c->ctl, c->bufs, c->XI2,
                                                                            nullptr, c->redpart, a.blocks, b.blocks,
                                                                            raocp::kDualAll, blk0);
        else
            raocp::k_cp_dual<false, NX, NU><<<grid, kBlock, 0, c->stream>>>(c->dev, c->ctl, c->bufs, c->XI2,
                                                                             dsolo, c->redpart, a.blocks, b.blocks, mode,
                                                                             blk0);
    }
};
void launch_cp_dual(raocp_ctx* c, bool with_l, double* dsolo, int mode = raocp::kDualAll, int role = 0) {
    dispatch(c->nx, c->nu, CpDualOp{}, c, with_l, dsolo, mode, role);
}

// One CP iteration for iteration index `it` within a graph batch. Graph batches are a
// multiple of 6 iterations and always start at k = 0 mod 6, so the buffer rotation
// Z[k % 3], E[k % 2] is static per captured node: the kernels get the buffers already
// rotated and never read the iteration counter to choose them.
raocp::Bufs rotated(raocp_ctx* c, int it) {
    return raocp::Bufs{c->Z[it % 3], c->Z[(it + 1) % 3], c->Z[(it + 2) % 3], c->E[it % 2], c->E[(it + 1) % 2]};
}

template <class T>
struct Cpd2Op {
    template <int RX, int RU>
    void run(raocp_ctx* c) {
        auto k = raocp::k_cpd2<T, RX, RU>;
        allow_lds(k, c->lds_cpd2);
        k<<<c->cp2_nbF + c->cp2_nbL, 64 * c->cp2_W, c->lds_cpd2, c->stream>>>(c->dev, c->ctl, c->bufs, c->XI2,
                                                                                c->redpart, c->cp2_nbF);
    }
};
template <class T>
struct Cpp2Op {
    template <int RX, int RU>
    void run(raocp_ctx* c) {
        auto k = raocp::k_cpp2<T, RX, RU>;
        allow_lds(k, c->lds_cpp2);
        k<<<c->cp2_nbF + c->cp2_nbL, 64 * c->cp2_W, c->lds_cpp2, c->stream>>>(c->dev, c->ctl, c->bufs, c->XI2,
                                                                                c->redpart, c->cp2_nbF);
    }
};
// the node-block kernels (raocp_cp.hip): fp64 at every size; fp32 contexts whose CP blocks
// mix weight tables (per-mode costs) at runtime sizes
template <class T>
struct CpdOp {
    template <int NX, int NU>
    void run(raocp_ctx* c) {
        auto k = raocp::k_cpd<T, NX, NU>;
        allow_lds(k, c->lds_cpd);
        k<<<c->cp_nbF + c->cp_nbL, kBlock, c->lds_cpd, c->stream>>>(c->dev, c->ctl, c->bufs, c->XI2, c->redpart,
                                                                     c->cp_nbF);
    }
};
template <class T>
struct CppOp {
    template <int NX, int NU>
    void run(raocp_ctx* c) {
        auto k = raocp::k_cpp<T, NX, NU>;
        allow_lds(k, c->lds_cpp);
        k<<<c->cp_nbF + c->cp_nbL, kBlock, c->lds_cpp, c->stream>>>(c->dev, c->ctl, c->bufs, c->XI2, c->redpart,
                                                                     c->cp_nbF);
    }
};
void launch_cpd(raocp_ctx* c) {
    if (c->f32 && c->cp_v1) CpdOp<float>{}.run<0, 0>(c);
    else if (c->f32) dispatch_rt(c->nx, c->nu, Cpd2Op<float>{}, c);
    else if (c->cp_v1) dispatch(c->nx, c->nu, CpdOp<double>{}, c);
    else dispatch_rt(c->nx, c->nu, Cpd2Op<double>{}, c);
}
void launch_cpp(raocp_ctx* c) {
    if (c->f32 && c->cp_v1) CppOp<float>{}.run<0, 0>(c);
    else if (c->f32) dispatch_rt(c->nx, c->nu, Cpp2Op<float>{}, c);
    else if (c->cp_v1) dispatch(c->nx, c->nu, CppOp<double>{}, c);
    else dispatch_rt(c->nx, c->nu, Cpp2Op<double>{}, c);
}
// the fused CP iteration (raocp_cp3.hip): compile-time sizes of the benchmark configs
// instantiated for the fp64 sizes of configs 2 and 4 and the fp32 sizes of configs 2, 4, 5
bool cp3_sizes(bool f32, int nx, int nu) {
    return (nx == 20 && nu == 8) || (nx == 32 && nu == 12) || (f32 && nx == 64 && nu == 16);
}
// a k_cp3 task list: split leaf tiles [l0, l1), then the parent ranges in order; returns
// the tiles, or -1 when the nonempty ranges exceed the kernel argument's kCp3MaxR slots (the
// caller must not launch it: a dropped range would leave its parents uncomputed)
long cp3_tasks(raocp::Cp3Tasks& tk, const std::vector<std::pair<int, int>>& ranges, int l0, int l1, int split,
               int mL, int gran = 16) {
    tk = raocp::Cp3Tasks{};
    tk.l0 = l0;
    tk.l1 = std::max(l0, l1);
    tk.split = split;
    tk.mL = mL;
    long tiles = (tk.l1 - tk.l0 + 15) / 16;
    for (const auto& r : ranges) {
        if (r.second <= r.first) continue;
        if (tk.nr >= raocp::kCp3MaxR) return -1;
        tk.lo[tk.nr] = r.first;
        tk.hi[tk.nr] = r.second;
        tk.t0[tk.nr + 1] = tk.t0[tk.nr] + (r.second - r.first + gran - 1) / gran;
        ++tk.nr;
    }
    if (tk.nr == 0) {  // an empty launch still needs one range (no tiles)
        tk.nr = 1;
        tk.t0[1] = 0;
    }
    return tiles + tk.t0[tk.nr];
}
int cp3_grid_of(long tiles) { return (int)std::max(1L, std::min((tiles + 3) / 4, 2048L)); }
// part 0: the unsharded launch, or a shard's first; 1: a shard's second (after X1), whose
// residual partials follow the first launch's rows
template <bool SH>
void launch_cp3t(raocp_ctx* c, int g, double* rp, const raocp::Cp3Tasks& tk) {
    const int C = c->unif_C, bx = c->box_mode;
    const double* im = c->cp3img;
    if (c->f32) {
        if (c->nx == 20) raocp::k_cp3<float, 20, 8, SH><<<g, 256, 0, c->stream>>>(c->dev, c->ctl, c->bufs, rp, c->XI2, C, bx, tk, im);
        else if (c->nx == 32) raocp::k_cp3<float, 32, 12, SH><<<g, 256, 0, c->stream>>>(c->dev, c->ctl, c->bufs, rp, c->XI2, C, bx, tk, im);
        else raocp::k_cp3<float, 64, 16, SH><<<g, 256, 0, c->stream>>>(c->dev, c->ctl, c->bufs, rp, c->XI2, C, bx, tk, im);
    } else {
        if (c->nx == 20) raocp::k_cp3<double, 20, 8, SH><<<g, 256, 0, c->stream>>>(c->dev, c->ctl, c->bufs, rp, c->XI2, C, bx, tk, im);
        else raocp::k_cp3<double, 32, 12, SH><<<g, 256, 0, c->stream>>>(c->dev, c->ctl, c->bufs, rp, c->XI2, C, bx, tk, im);
    }
}
// k_cp3's weight image (one workgroup, at context creation)
template <class T, int NX, int NU>
int cp3_imaget(raocp_ctx* c) {
    typedef raocp::WL<T, NX, NX> WQ;
    typedef raocp::WL<T, NU, NU> WR;
    int rc;
    if ((rc = c->alloc(&c->cp3img, (size_t)(2 * WQ::N + WR::N) * sizeof(T) / 8))) return rc;
    raocp::k_cp3_image<T, NX, NU><<<1, 256, 0, c->stream>>>(c->dev, c->cp3img);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return RAOCP_OK;
}
int cp3_image(raocp_ctx* c) {
    if (c->f32) {
        if (c->nx == 20) return cp3_imaget<float, 20, 8>(c);
        if (c->nx == 32) return cp3_imaget<float, 32, 12>(c);
        return cp3_imaget<float, 64, 16>(c);
    }
    if (c->nx == 20) return cp3_imaget<double, 20, 8>(c);
    return cp3_imaget<double, 32, 12>(c);
}
// the CP iteration after the dynamics in its fused form (cp_fused(c->path.cp)); sh: a shard's ranges and task lists
void launch_cp_fused(raocp_ctx* c, int part = 0) {
    const bool sh = c->sh_S > 0;
    switch (c->path.cp) {
        case CpPath::Cp6:
            raocp::cp6_launch(c->dev, c->ctl, c->bufs, c->redpart, c->box_mode, c->cp5_tk, c->cp6_grid, c->cp3img, c->stream);
            return;
        case CpPath::Cp5:
            // a shard: its eta2 tasks, leaves and families, then (part 1, after X1) the cut's parents
            if (part == 0)
                raocp::cp5_launch(c->dev, c->ctl, c->bufs, c->redpart, c->unif_C, c->box_mode, c->cp5_et,
                                  sh ? c->own_lo[c->N] : c->m, sh ? c->own_hi[c->N] : c->n, c->cp5_gl, c->cp5_tk, c->cp5_gf,
                                  c->cp3img, c->cp5_lpf, c->stream);
            else
                raocp::cp5_launch(c->dev, c->ctl, c->bufs, c->redpart + (size_t)raocp::cp5_rows(c->cp5_gl, c->cp5_gf) * 6,
                                  c->unif_C, c->box_mode, c->cp5_et, 0, 0, 0, c->cp5_tkb, c->cp5_gfb, c->cp3img, c->cp5_lpf,
                                  c->stream);
            return;
        case CpPath::Cp4:
            raocp::cp4_launch(c->dev, c->ctl, c->bufs, c->redpart, c->unif_C, c->box_mode, c->cp3_ta, c->cp3img, c->cp3_grid,
                              c->cp4_wpb, c->stream);
            return;
        case CpPath::Cp3:
            if (sh)
                launch_cp3t<true>(c, part ? c->cp3_gridb : c->cp3_grid, c->redpart + (part ? (size_t)c->cp3_grid * 6 : 0),
                                  part ? c->cp3_tb : c->cp3_ta);
            else
                launch_cp3t<false>(c, c->cp3_grid, c->redpart, c->cp3_ta);
            return;
        default: return;  // not a fused form: launch_cp_after_sweep
    }
}
// the CP kernels after the sweep: the fused form, or k_cpd* then k_cpp*. half 0: all of it; a
// shard launches half 1 before its X1 exchange and half 2 after it
void launch_cp_after_sweep(raocp_ctx* c, int half = 0) {
    if (raocp::cp_fused(c->path.cp)) return launch_cp_fused(c, half == 2 ? 1 : 0);
    if (half != 2) launch_cpd(c);
    if (half != 1) launch_cpp(c);
}
// the solve's first half step Z[1] = prox-part(Z[0] - alpha L^T E[0]) (s_0 relaxation,
// kernel projection): k_cp_primal; an fp32 context runs k_cpp2 on {p = z+ = Z[0], d = eta+ =
// E[0]} (its residual partials are overwritten by iteration 0 before they are read)
void launch_first_half(raocp_ctx* c) {
    if (!c->f32) {
        launch_cp_primal(c, false);
        return;
    }
    const raocp::Bufs keep = c->bufs;
    c->bufs = raocp::Bufs{c->Z[0], c->Z[0], c->Z[1], c->E[0], c->E[0]};
    launch_cpp(c);
    c->bufs = keep;
}
// Deferred stopping test (default for the tiered dynamics; RAOCP_DEFER_CHECK=0 disables):
// iteration k's test runs in an extra workgroup of iteration k + 1's first dynamics launch
// instead of its own k_cp_check launch after k_cpp, and a batch ends with one k_cp_check
// for its last iteration. Iteration k + 1's kernels that start before the test fires only
// write the next iterate's buffers (Z[(k + 1) % 3] projected in place, nothing of
// z+_k = Z[k % 3] or eta+_k = E[k % 2]), and every later kernel exits on ctl->done, so the
// result and the history are those of the eager test.
bool defer_check(const raocp_ctx* c) {
    if (c->comm || c->sh_R != 1 || c->no_defer_check) return false;
    switch (c->path.dyn) {  // the sweeps whose first launch can carry the test
        case DynPath::Dr: return true;
        case DynPath::Dyn3: return c->N >= 1;
        case DynPath::TiersSplit:
        case DynPath::Tiers: return !c->tiers.empty() && c->tiers.back().nsub > 0;
        default: return false;
    }
}

// ---- RCCL, loaded on demand (dlopen) so single-GPU users never load it
struct Rccl {
    void* h = nullptr;
    ncclResult_t (*get_id)(ncclUniqueId*) = nullptr;
    ncclResult_t (*init_rank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*all_gather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*all_reduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*destroy)(ncclComm_t) = nullptr;
    const char* (*err)(ncclResult_t) = nullptr;
};
Rccl g_rccl;
int rccl_load() {
    if (g_rccl.h) return RAOCP_OK;
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return fail(RAOCP_ERR_HIP, std::string("cannot load librccl: ") + dlerror());
    g_rccl.get_id = (decltype(g_rccl.get_id))dlsym(h, "ncclGetUniqueId");
    g_rccl.init_rank = (decltype(g_rccl.init_rank))dlsym(h, "ncclCommInitRank");
    g_rccl.all_gather = (decltype(g_rccl.all_gather))dlsym(h, "ncclAllGather");
    g_rccl.all_reduce = (decltype(g_rccl.all_reduce))dlsym(h, "ncclAllReduce");
    g_rccl.destroy = (decltype(g_rccl.destroy))dlsym(h, "ncclCommDestroy");
    g_rccl.err = (decltype(g_rccl.err))dlsym(h, "ncclGetErrorString");
    if (!g_rccl.get_id || !g_rccl.init_rank || !g_rccl.all_gather || !g_rccl.all_reduce || !g_rccl.destroy)
        return fail(RAOCP_ERR_HIP, "librccl lacks the collectives used here");
    g_rccl.h = h;
    return RAOCP_OK;
}

// The two exchanges of a sharded iteration:
//   X2  after the tiers' backward sweeps: q rows of the boundary roots (all-gather);
//   X1  after k_cpd: eta+ and xi2 of the roots' eta2 (all-gather), read by the
//       replicated top families of k_cpp, carrying the previous iteration's 16-double
//       residual record too (k_cp_reduce after k_cpp packs it; the stopping test runs one
//       iteration late, k_cp_check_gather), so SURVEY.md's X3 all-reduce is not needed.
// pack/unpack run on every shard; the collective itself is RCCL, or, for shards that
// share a process (raocp_group_cp_run), host-driven copies between the phases.
// X2 rows: the tiered sweep's q rows (KP doubles each), or the per-stage sweep's (nx scalars
// of the context's type, raocp_dyn3.hip)
bool x2_dyn3(const raocp_ctx* c) { return c->path.dyn == DynPath::Dyn3; }
int x2_row(const raocp_ctx* c) { return x2_dyn3(c) ? c->nx : c->KP; }
int x2_elt(const raocp_ctx* c) { return x2_dyn3(c) ? c->wsz : 8; }
double* x2_q(const raocp_ctx* c) { return x2_dyn3(c) ? c->Q2 : c->q; }
size_t x2_bytes(const raocp_ctx* c) { return (size_t)c->x_max * x2_row(c) * x2_elt(c); }
void shard_pack_x2(raocp_ctx* c) {
    const size_t row = (size_t)x2_row(c) * x2_elt(c);
    if (c->own_cnt)
        (void)hipMemcpyAsync(c->x2_send, (char*)x2_q(c) + (size_t)c->own_first * row, (size_t)c->own_cnt * row,
                             hipMemcpyDeviceToDevice, c->stream);
}
void shard_unpack_x2(raocp_ctx* c) {
    const int tot = c->sh_R * c->x_max * x2_row(c);
    const int g = std::max(1, std::min(256, cdiv(tot, kBlock)));
    if (x2_elt(c) == 4)
        raocp::k_scatter_rows<float><<<g, kBlock, 0, c->stream>>>((const float*)c->x2_recv, (float*)x2_q(c), c->d_slc,
                                                                   c->sh_R, c->x_max, x2_row(c));
    else
        raocp::k_scatter_rows<double><<<g, kBlock, 0, c->stream>>>(c->x2_recv, x2_q(c), c->d_slc, c->sh_R, c->x_max,
                                                                    x2_row(c));
}
// X1 carries two entries per root and the previous iteration's residual record: under k_cp3
// the roots' (eta+, xi2) eta2 entries, under k_cp5 the roots' s of the half step before their
// parents' kernel projection (k_cp5_leaf's eta2 tasks write it, the cut's parents' family tiles
// read it) and eta+ of their eta2
int x1_len(const raocp_ctx* c) { return 2 * c->x_max + 16; }
struct X1Src {
    double *a, *b;  // buffers (of the context's type) and element offsets of root 0's entries
    int oa, ob;
};
X1Src x1_src(const raocp_ctx* c) {
    if (c->path.cp == CpPath::Cp5) return X1Src{c->bufs.z2, c->bufs.e1, c->dev.S0, c->dev.E2};
    return X1Src{c->bufs.e1, c->XI2, c->dev.E2, c->dev.E2};
}
void shard_pack_x1(raocp_ctx* c) {
    const int g = std::max(1, cdiv(c->own_cnt, kBlock)), o = c->own_first;
    const X1Src x = x1_src(c);
    if (c->f32)
        raocp::k_pack_x1<float><<<g, kBlock, 0, c->stream>>>(c->x1_send, (const float*)x.a + x.oa + o,
                                                             (const float*)x.b + x.ob + o, c->own_cnt, c->x_max, c->red8);
    else
        raocp::k_pack_x1<double><<<g, kBlock, 0, c->stream>>>(c->x1_send, x.a + x.oa + o, x.b + x.ob + o, c->own_cnt,
                                                              c->x_max, c->red8);
}
void shard_unpack_x1(raocp_ctx* c) {
    const int g = std::max(1, cdiv(c->sh_R * c->x_max, kBlock));
    const X1Src x = x1_src(c);
    if (c->f32)
        raocp::k_unpack_x1<float><<<g, kBlock, 0, c->stream>>>(c->x1_recv, (float*)x.a + x.oa, (float*)x.b + x.ob, c->d_slc,
                                                               c->sh_R, c->x_max);
    else
        raocp::k_unpack_x1<double><<<g, kBlock, 0, c->stream>>>(c->x1_recv, x.a + x.oa, x.b + x.ob, c->d_slc, c->sh_R,
                                                                c->x_max);
    raocp::k_cp_check_gather<<<1, 64, 0, c->stream>>>(c->ctl, c->hist, c->x1_recv, c->sh_R, c->x_max);
}
int rccl_check(ncclResult_t r, const char* what) {
    if (r != ncclSuccess)
        return fail(RAOCP_ERR_HIP, std::string(what) + ": " + (g_rccl.err ? g_rccl.err(r) : "rccl error"));
    return RAOCP_OK;
}

// the three phases of a shard's CP iteration; the transport (RCCL in enqueue_shard_iteration, device copies in
// raocp_group_cp_run) moves x2_send -> x2_recv after the first and x1_send -> x1_recv after the second
void shard_phase_back(raocp_ctx* c) {  // the backward sweep below the cut, its roots' q rows packed
    launch_dynamics(c, c->bufs, 1, c->ctl, 1);
    shard_pack_x2(c);
}
void shard_phase_fwd(raocp_ctx* c) {  // the top and the forward sweep, the first CP launch, X1 packed
    shard_unpack_x2(c);
    launch_dynamics(c, c->bufs, 1, c->ctl, 2);
    launch_cp_after_sweep(c, 1);
    shard_pack_x1(c);
}
void shard_phase_top(raocp_ctx* c) {  // the second CP launch (the previous iteration's stopping test first)
    shard_unpack_x1(c);
    launch_cp_after_sweep(c, 2);
    raocp::k_cp_reduce<<<1, kBlock, 0, c->stream>>>(c->ctl, c->redpart, c->cp_rows, c->red8);
}

// one CP iteration of a shard whose transport is RCCL (graph-capturable)
int enqueue_shard_iteration(raocp_ctx* c) {
    ncclComm_t comm = (ncclComm_t)c->comm;
    int rc;
    shard_phase_back(c);
    if ((rc = rccl_check(g_rccl.all_gather(c->x2_send, c->x2_recv, (size_t)c->x_max * x2_row(c),
                                           x2_elt(c) == 4 ? ncclFloat32 : ncclFloat64, comm, c->stream),
                         "ncclAllGather(q)")))
        return rc;
    shard_phase_fwd(c);
    if ((rc = rccl_check(g_rccl.all_gather(c->x1_send, c->x1_recv, (size_t)x1_len(c), ncclFloat64, comm, c->stream),
                         "ncclAllGather(eta2, residuals)")))
        return rc;
    shard_phase_top(c);
    return RAOCP_OK;
}

// the last iteration's stopping test (its record has no next iteration to ride on): the
// X1 all-gather with only the residual record meaningful
int enqueue_shard_tail(raocp_ctx* c) {
    shard_pack_x1(c);
    int rc;
    if ((rc = rccl_check(g_rccl.all_gather(c->x1_send, c->x1_recv, (size_t)x1_len(c), ncclFloat64, (ncclComm_t)c->comm,
                                           c->stream),
                         "ncclAllGather(residuals)")))
        return rc;
    raocp::k_cp_check_gather<<<1, 64, 0, c->stream>>>(c->ctl, c->hist, c->x1_recv, c->sh_R, c->x_max);
    return RAOCP_OK;
}

// k_drc's residual rows of iteration parity q, and the ctl->flags bit of its NaN-in-box flag
double* drc_part(raocp_ctx* c, int q) { return c->redpart + (size_t)(q & 1) * c->cp_rows * 6; }
int drc_nanbit(int q) { return 2 << (q & 1); }
// the fused launch of iteration `it` (k = it mod 2 within a batch that starts at k = 0 mod 6)
void launch_drc(raocp_ctx* c, int it, bool with_check) {
    raocp::DrPlan p = c->drp;
    if (c->dev.stamps) p.stamps = c->dev.stamps;
    const raocp::ChkArg ck{c->ctl, c->hist, drc_part(c, it - 1), c->cp_rows, with_check ? 1 : 0, drc_nanbit(it - 1)};
    raocp::drc_launch(p, c->d_drca + (it & 1), c->drca.box, c->drc_lds, c->bufs, ck, c->stream);
}
// iteration `it`'s stopping test as a launch of its own (k_drc's residual rows and NaN bit go by parity)
void launch_cp_check(raocp_ctx* c, int it, raocp::CtlPub* pub, const unsigned* ew) {
    const bool f = c->path.fused;
    raocp::k_cp_check<<<1, kBlock, 0, c->stream>>>(c->ctl, c->hist, f ? drc_part(c, it) : c->redpart, c->cp_rows,
                                                   f ? drc_nanbit(it) : 0, pub, ew);
}
int enqueue_cp_iteration(raocp_ctx* c, int it) {
    const raocp::Bufs keep = c->bufs;
    c->bufs = rotated(c, it);
    if (c->comm) {
        const int rc = enqueue_shard_iteration(c);
        c->bufs = keep;
        return rc;
    }
    const bool defer = defer_check(c);
    if (c->path.fused) {
        launch_drc(c, it, defer && it > 0);
    } else {
        const raocp::ChkArg ck{c->ctl, c->hist, c->redpart, c->cp_rows, 1};
        launch_dynamics(c, c->bufs, 1, c->ctl, 0, defer && it > 0 ? &ck : nullptr);
        launch_cp_after_sweep(c);
    }
    c->bufs = keep;
    if (!defer) launch_cp_check(c, it, nullptr, nullptr);
    return RAOCP_OK;
}
// the kernel the default selection launches for op (raocp_op_bench numbering: 0 L, 1 L^T,
// 2 dual CP kernel, 6 primal CP kernel, 9 the dynamics projection), as rocprofv3 names it
std::string kernel_name(const raocp_ctx* c, int op) {
    const std::string T = c->f32 ? "float" : "double";
    const bool exact = (c->nx == 20 && c->nu == 8) || (c->nx == 32 && c->nu == 12) || (c->nx == 64 && c->nu == 16) ||
                       (c->nx == 3 && c->nu == 2);
    const std::string nn = exact ? std::to_string(c->nx) + ", " + std::to_string(c->nu) : "0, 0";
    const int rx = std::min(4, (c->nx + 15) / 16), ru = c->nu <= 16 ? 1 : 2;
    const std::string rr = std::to_string(rx) + ", " + std::to_string(ru);
    const bool big = (c->nx == 20 && c->nu == 8) || (c->nx == 32 && c->nu == 12) || (c->nx == 64 && c->nu == 16);
    switch (op) {
        case 0:
            if (c->ell3 && big) return "k_ell3<" + T + ", " + nn + ">";
            return c->f32 ? "k_ell2<float, " + rr + ">" : "k_ell<" + nn + ">";
        case 1:
            if (c->ellt3_C && big) return "k_ellt3<" + T + ", " + nn + ", " + std::to_string(4 / c->ellt3_C) + ">";
            return c->f32 ? "k_ellt2<float, " + rr + ">" : "k_ell_t<" + nn + ">";
        case 2:
            if (c->cp_v1) return "k_cpd<" + T + ", " + (c->f32 ? std::string("0, 0") : nn) + ">";
            return "k_cpd2<" + T + ", " + rr + ">";
        case 6:
            if (c->cp_v1) return "k_cpp<" + T + ", " + (c->f32 ? std::string("0, 0") : nn) + ">";
            return "k_cpp2<" + T + ", " + rr + ">";
        case 9: {
            // the launches of one projection as "name xcount" terms (bench.py sums the PMC
            // traffic of these terms)
            std::vector<std::pair<std::string, int>> terms;
            auto add = [&](const std::string& k) {
                for (auto& t : terms)
                    if (t.first == k) {
                        ++t.second;
                        return;
                    }
                terms.push_back({k, 1});
            };
            auto b = [](bool v) { return std::string(v ? "true" : "false"); };
            switch (c->path.dyn) {
                case DynPath::Dr: return std::string(raocp::dr_name(c->nx, c->nu)) + " x1";
                case DynPath::Dyn3: {  // a backward and a forward launch per nonleaf stage below the top
                    const int ts = dyn3_top_stages(c);
                    for (int t = ts; t < c->N; ++t) add("k_dy3_back<" + T + ", " + nn + ">");
                    if (ts) add("k_dy3_top_back<" + T + ", " + nn + ">");
                    if (ts) add("k_dy3_top_fwd<" + T + ", " + nn + ">");
                    for (int t = ts; t < c->N; ++t) add("k_dy3_fwd<" + T + ", " + nn + ">");
                    break;
                }
                case DynPath::Dyn2: return "k_d2_prod + k_d2_node + k_d2_x0 + k_d2_fwd (per stage, " + T + ")";
                case DynPath::TiersSplit:
                    return "k_dyn_up<" + nn + "> x1 + k_dyn_down<" + nn + ", " + b(c->f_lds_top) + "> x1";
                case DynPath::Tiers:
                    for (int k = (int)c->tiers.size() - 1; k >= 0; --k)
                        add("k_dyn_bottom_back<" + nn + ", " + b(c->tiers[k].fold) + ">");
                    add("k_dyn_top<" + nn + ", " + b(c->f_lds_top) + ", " + b(c->fold_top) + ">");
                    for (const auto& tp : c->tiers) add("k_dyn_bottom_fwd<" + nn + ", " + std::to_string(tp.fm) + ">");
                    break;
                case DynPath::PerStage: return "k_dyn_gather + k_dyn_stage_a / _b / _f (per stage)";
            }
            std::string s;
            for (const auto& t : terms) s += (s.empty() ? "" : " + ") + t.first + " x" + std::to_string(t.second);
            return s;
        }
        case 11:  // the CP loop's fused launch (dynamics projection + CP iteration), if any
            return c->path.fused ? raocp::drc_name() : "";
        case 15:    // the composed maps of the regular-tree sweep that are active ("" when none)
        case 16: {  // ... its composed forward maps
            std::string s;
            for (int k = 0; k < c->drp.T && c->path.dyn == DynPath::Dr; ++k) {
                const char* m = op == 15 ? "mid_back_root@" : (k == c->drp.T - 1 ? "deep_fwd@" : "mid_fwd@");
                if (c->drp.t[k].xf & (op == 15 ? raocp::kDrXfMidBack : raocp::kDrXfFwd)) s += (s.empty() ? "" : " ") + std::string(m) + std::to_string(k);
            }
            return s;
        }
        case 12:  // the forms of the k_cp5 launches, when they run ("" otherwise)
            if (c->path.cp != CpPath::Cp5) return "";
            return std::string("leaf_pf=") + (c->cp5_lpf ? "1" : "0");
        case 13:  // the batched CP kernel, when raocp_cp_batch_run launches it ("" otherwise)
            return cpb_on(c) ? raocp::cpb_name(c->f32, raocp::cpb_tab_bytes(c->dev, c->f32) > 0) : "";
        case 19:  // the accelerated batch kernel of raocp_cp_batch_run_aa ("" where it refuses)
            return cpb_on(c) && !c->f32 ? raocp::cpa_name(raocp::cpb_tab_bytes(c->dev, false) > 0) : "";
        case 14:  // the step kernel of raocp_cp_batch_mpc ("" when the loop runs on the host)
            return cpb_on(c) ? raocp::mpc_step_name(c->f32) : "";
        case 20:  // the step kernel of raocp_cp_batch_mpc_aa ("" where it refuses)
            return cpb_on(c) && !c->f32 ? raocp::mpc_step_aa_name() : "";
        case 17:  // the kernels of raocp_evaluate and its number of sweep launches
            return raocp::eval_name(c->f32, (int)raocp::eval_sweep_plan(c->stage_ptr).size());
        case 18:  // the kernel of raocp_cp_batch_evaluate: the last batch's own form, else what a batch would run
            return (c->bt.B >= 1 ? c->bt.kernel : cpb_on(c)) ? raocp::eval_batch_name(c->f32) : "";
        case 10: {  // a shard launches the fused forms k_cp5 and k_cp3 twice (launch_cp_fused)
            const bool sh = c->sh_S > 0;
            switch (c->path.cp) {
                case CpPath::Cp6: return raocp::cp6_name();
                case CpPath::Cp5: return std::string(raocp::cp5_name(c->f32, c->nx)) + (sh ? " (+ fams x1 after X1)" : "");
                case CpPath::Cp4: return raocp::cp4_name(c->f32, c->nx, c->nu);
                case CpPath::Cp3: return "k_cp3<" + T + ", " + nn + (sh ? ", true> x2" : ", false>");
                default: return kernel_name(c, 2) + " + " + kernel_name(c, 6);
            }
        }
        default: return "";
    }
}

// the end of a batch of `iters` iterations: the deferred test of its last iteration
void enqueue_batch_tail(raocp_ctx* c, int iters) {
    if (defer_check(c)) launch_cp_check(c, iters - 1, c->d_pub, err_word(c));
}

int set_ctl_alpha(raocp_ctx* c, double alpha) {
    HIPCHK(hipMemcpyAsync(&c->ctl->alpha, &alpha, sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return RAOCP_OK;
}

// what the context runs, from what was set up (raocp_path.h): at the end of raocp_ctx_create, and again at the
// end of raocp_shard_setup, whose cut takes a shard off the forms that span the whole tree
void resolve_ctx_paths(raocp_ctx* c) {
    const raocp::PathCaps k{c->cp3, c->cp4, c->cp5,  c->cp6,  c->cp_v1,     c->dr,
                            c->drc, c->dyn2, c->dyn3, c->dyn_split, c->cut > 0};  // PathCaps' order
    c->path = raocp::resolve_paths(k, c->sh_S > 0);
}

void drop_graphs(raocp_ctx* c) {
    if (c->graph) (void)hipGraphExecDestroy(c->graph);
    if (c->graph_rem) (void)hipGraphExecDestroy(c->graph_rem);
    c->graph = c->graph_rem = nullptr;
    c->graph_iters = c->graph_rem_iters = 0;
}

int ensure_hist(raocp_ctx* c, size_t rows) {
    if (rows <= c->hist_rows) return RAOCP_OK;
    if (c->hist) {
        (void)hipFree(c->hist);
        c->allocs.erase(std::remove(c->allocs.begin(), c->allocs.end(), (void*)c->hist), c->allocs.end());
        c->hist = nullptr;
    }
    int rc = c->alloc(&c->hist, rows * 6);
    if (rc) return rc;
    c->hist_rows = rows;
    drop_graphs(c);  // the graphs reference the history buffer
    return RAOCP_OK;
}

// Prepare a CP run: the starting primal / dual go to Z[0] / E[0] and ctl is reset.
// warm: start from the context's current primal / dual (the reference's chock continues
// from the cached old primal / dual, solver.py:27-61 with cache.py:58-66, 186-196), with
// x0 written into node 0's state (cache_initial_state, cache.py:79-82); otherwise from
// (x0 at node 0, zeros) / 0.
int cp_init(raocp_ctx* c, const double* x0, int max_iters, double tol, double alpha, bool warm = false) {
    if (warm) {
        if (c->cur_z != c->Z[0])
            HIPCHK(hipMemcpyAsync(c->Z[0], c->cur_z, c->P * c->wsz, hipMemcpyDeviceToDevice, c->stream));
        if (c->cur_e != c->E[0])
            HIPCHK(hipMemcpyAsync(c->E[0], c->cur_e, c->D * c->wsz, hipMemcpyDeviceToDevice, c->stream));
    } else {
        HIPCHK(hipMemsetAsync(c->Z[0], 0, c->P * sizeof(double), c->stream));
        HIPCHK(hipMemsetAsync(c->E[0], 0, c->D * sizeof(double), c->stream));
    }
    if (c->red8) HIPCHK(hipMemsetAsync(c->red8, 0, 16 * sizeof(double), c->stream));  // no previous record
    for (int b = 1; b < 3; ++b) HIPCHK(hipMemsetAsync(c->Z[b], 0, c->P * sizeof(double), c->stream));
    HIPCHK(hipMemsetAsync(c->E[1], 0, c->D * sizeof(double), c->stream));
    HIPCHK(hipMemsetAsync(c->XI2, 0, c->D * sizeof(double), c->stream));
    if (c->f32) {
        const std::vector<float> f(x0, x0 + c->nx);
        HIPCHK(hipMemcpyAsync((float*)c->Z[0] + c->dev.X0, f.data(), c->nx * sizeof(float), hipMemcpyHostToDevice,
                              c->stream));
        HIPCHK(hipMemcpyAsync(c->x0, f.data(), c->nx * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));  // f leaves scope
    } else {
        HIPCHK(hipMemcpyAsync(c->Z[0] + c->dev.X0, x0, c->nx * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(c->x0, x0, c->nx * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    Ctl h{};
    h.alpha = alpha;
    h.k = 0;
    h.done = 0;
    h.final_k = -1;
    h.flags = 0;
    h.max_iters = max_iters;
    h.tol = tol;
    *c->h_ctl = h;
    HIPCHK(hipMemcpyAsync(c->ctl, c->h_ctl, sizeof(Ctl), hipMemcpyHostToDevice, c->stream));
    launch_first_half(c);
    return RAOCP_OK;
}

// the captured batch of `iters` CP iterations: kGraphBatch in the main slot, any other
// count (a benchmark's remainder, always launched after whole batches, so it also starts
// at k = 0 mod 6) in the remainder slot
int ensure_graph(raocp_ctx* c, int iters) {
    if (c->eager) return RAOCP_OK;
    const bool rem = iters != kGraphBatch;
    hipGraphExec_t& slot = rem ? c->graph_rem : c->graph;
    int& slot_iters = rem ? c->graph_rem_iters : c->graph_iters;
    if (slot && slot_iters == iters) return RAOCP_OK;
    if (slot) {
        (void)hipGraphExecDestroy(slot);
        slot = nullptr;
    }
    hipGraph_t g = nullptr;
    HIPCHK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    int rc_enq = RAOCP_OK;
    for (int it = 0; it < iters && rc_enq == RAOCP_OK; ++it) rc_enq = enqueue_cp_iteration(c, it);
    if (rc_enq == RAOCP_OK) enqueue_batch_tail(c, iters);
    hipError_t e = hipStreamEndCapture(c->stream, &g);
    if (rc_enq != RAOCP_OK) {
        if (g) (void)hipGraphDestroy(g);
        (void)hipGetLastError();
        if (!c->comm) return rc_enq;
        // an RCCL shard whose collectives cannot be captured: launch iterations eagerly
        c->eager = true;
        return RAOCP_OK;
    }
    if (e == hipSuccess) {
        e = hipGraphInstantiate(&slot, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        // the executable graph's device-side setup now, not inside its first (timed) launch
        if (e == hipSuccess) e = hipGraphUpload(slot, c->stream);
    }
    if (e != hipSuccess) {
        if (!c->comm) return fail(RAOCP_ERR_HIP, std::string("graph capture: ") + hipGetErrorString(e));
        // an RCCL shard whose collectives cannot be captured: launch iterations eagerly
        (void)hipGetLastError();
        slot = nullptr;
        c->eager = true;
        return RAOCP_OK;
    }
    slot_iters = iters;
    return RAOCP_OK;
}

// launch one batch of `iters` CP iterations (the captured graph, or eagerly)
int launch_batch(raocp_ctx* c, int iters) {
    if (c->eager) {
        for (int it = 0; it < iters; ++it) {
            const int rc = enqueue_cp_iteration(c, it);
            if (rc) return rc;
        }
        enqueue_batch_tail(c, iters);
        HIPCHK(hipGetLastError());
        return RAOCP_OK;
    }
    HIPCHK(hipGraphLaunch(iters == kGraphBatch ? c->graph : c->graph_rem, c->stream));
    return RAOCP_OK;
}

// the residual history of a finished run (rows 0 .. fk) into the caller's arrays
int copy_hist(raocp_ctx* c, int fk, double* err_hist, double* delta_hist) {
    std::vector<double> h((size_t)(fk + 1) * 6);
    HIPCHK(hipMemcpy(h.data(), c->hist, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int k = 0; k <= fk; ++k)
        for (int q = 0; q < 3; ++q) {
            if (err_hist) err_hist[k * 3 + q] = h[(size_t)k * 6 + q];
            if (delta_hist) delta_hist[k * 3 + q] = h[(size_t)k * 6 + 3 + q];
        }
    return RAOCP_OK;
}
// random inputs (seed 1) in the staging buffers tmpP / tmpD (raocp_op_bench, raocp_op_bench_rot)
int bench_inputs(raocp_ctx* c) {
    std::vector<double> hz(c->P), he(c->D);
    std::mt19937_64 gen(1);
    std::normal_distribution<double> nd(0.0, 1.0);
    for (auto& v : hz) v = nd(gen);
    for (auto& v : he) v = nd(gen);
    int rc = copy_in(c, c->tmpP, hz.data(), c->P, 0);
    return rc ? rc : copy_in(c, c->tmpD, he.data(), c->D, 0);
}

}  // namespace

#include "raocp_setup.h"

extern "C" {

const char* raocp_last_error(void) { return raocp::g_err.c_str(); }

int raocp_device_synchronize(int device) {
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipDeviceSynchronize());
    return RAOCP_OK;
}

int raocp_ctx_create(const raocp_tree_desc* t, const raocp_problem_desc* pr, int device, raocp_ctx** out) {
    if (!t || !pr || !out) return fail(RAOCP_ERR_ARG, "null argument");
    *out = nullptr;
    int N = 0, cmax = 0, rc;
    if ((rc = validate_tree(t, &N, &cmax))) return rc;  // before any HIP call

    int prev_dev = -1;
    (void)hipGetDevice(&prev_dev);
    HIPCHK(hipSetDevice(device));
    struct Restore {
        int d;
        ~Restore() { if (d >= 0) (void)hipSetDevice(d); }
    } restore_{prev_dev != device ? prev_dev : -1};
    if (pr->dtype != RAOCP_F64 && pr->dtype != RAOCP_F32) return fail(RAOCP_ERR_ARG, "dtype must be RAOCP_F64 or RAOCP_F32");
    raocp_ctx* c = new raocp_ctx();
    c->device = device;
    c->n = t->n; c->m = t->m; c->nx = t->nx; c->nu = t->nu; c->cmax = cmax; c->N = N;
    c->f32 = pr->dtype == RAOCP_F32;
    c->wsz = c->f32 ? 4 : 8;
    auto bail = [&](int code) { raocp_ctx_destroy(c); return code; };
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess)
        return bail(fail(RAOCP_ERR_HIP, "hipStreamCreate failed"));
    const int n_cus = device_cus(device);
    Layout lay;     // host tables the later stages read (raocp_setup.h)
    DynTables dt;
    if ((rc = layout_vectors(c, t, pr, lay))) return bail(rc);
    if ((rc = upload_cost_tables(c, t, pr, lay))) return bail(rc);
    if ((rc = build_dyn_tables(c, t, pr, dt))) return bail(rc);
    if ((rc = setup_dyn3_dyn2(c, t, pr, dt))) return bail(rc);
    if ((rc = setup_dr(c, dt, n_cus))) return bail(rc);
    if ((rc = upload_node_records(c, t, pr, dt))) return bail(rc);
    const raocp::TierPlanResult plan = plan_dyn_tiers(c, t, dt, n_cus);
    if ((rc = build_tier_plans(c, t, plan))) return bail(rc);
    if ((rc = setup_split_sweep(c, dt, n_cus))) return bail(rc);
    if ((rc = setup_cp_blocks(c, t, pr, lay))) return bail(rc);
    if ((rc = setup_ell_blocks(c, t, pr))) return bail(rc);
    if ((rc = alloc_iterate(c))) return bail(rc);
    if ((rc = choose_streaming_kernels(c, t, pr))) return bail(rc);
    if ((rc = drc_setup(c, n_cus))) return bail(rc);
    c->no_defer_check = !env_flag("RAOCP_DEFER_CHECK", true);
    c->drp.zpage = c->dev.zpage;
    c->drp.x0 = c->x0;
    resolve_ctx_paths(c);
    *out = c;
    return RAOCP_OK;
}

void raocp_ctx_destroy(raocp_ctx* c) {
    if (!c) return;
    DevGuard dg_(c);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->comm && g_rccl.destroy) (void)g_rccl.destroy((ncclComm_t)c->comm);
    drop_graphs(c);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    for (void* p : c->allocs) (void)hipFree(p);
    batch_free(c);
    mpc_free(c);
    if (c->h_ctl) (void)hipHostFree(c->h_ctl);
    if (c->h_pub) (void)hipHostFree(c->h_pub);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int raocp_sizes(raocp_ctx* c, int64_t* P, int64_t* D) {
    DevGuard dg_(c);
    if (!c) return fail(RAOCP_ERR_ARG, "null context");
    if (P) *P = c->P;
    if (D) *D = c->D;
    return RAOCP_OK;
}

int raocp_ell(raocp_ctx* c, const double* z, double* eta, int flags) {
    DevGuard dg_(c);
    if (!c || !z || !eta) return fail(RAOCP_ERR_ARG, "null argument");
    int rc;
    if ((rc = ell_available(c))) return rc;
    if (flags & RAOCP_DEVICE_PTR) {
        launch_ell(c, z, eta);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(c->stream));
        return RAOCP_OK;
    }
    if ((rc = copy_in(c, c->tmpP, z, c->P, 0)) || (rc = copy_in(c, c->tmpD, eta, c->D, 0))) return rc;
    launch_ell(c, c->tmpP, c->tmpD);
    HIPCHK(hipGetLastError());
    return copy_out(c, eta, c->tmpD, c->D, 0);
}

int raocp_ell_t(raocp_ctx* c, const double* eta, double* z, int flags) {
    DevGuard dg_(c);
    if (!c || !z || !eta) return fail(RAOCP_ERR_ARG, "null argument");
    int rc;
    if ((rc = ell_available(c))) return rc;
    if (flags & RAOCP_DEVICE_PTR) {
        launch_ell_t(c, eta, z);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(c->stream));
        return RAOCP_OK;
    }
    if ((rc = copy_in(c, c->tmpD, eta, c->D, 0)) || (rc = copy_in(c, c->tmpP, z, c->P, 0))) return rc;
    launch_ell_t(c, c->tmpD, c->tmpP);
    HIPCHK(hipGetLastError());
    return copy_out(c, z, c->tmpP, c->P, 0);
}

int raocp_set_primal(raocp_ctx* c, const double* z, int flags) {
    DevGuard dg_(c);
    if (!c || !z) return fail(RAOCP_ERR_ARG, "null argument");
    int rc = copy_in(c, c->cur_z, z, c->P, flags);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return RAOCP_OK;
}
int raocp_get_primal(raocp_ctx* c, double* z, int flags) {
    DevGuard dg_(c);
    if (!c || !z) return fail(RAOCP_ERR_ARG, "null argument");
    return copy_out(c, z, c->cur_z, c->P, flags);
}
int raocp_set_dual(raocp_ctx* c, const double* e, int flags) {
    DevGuard dg_(c);
    if (!c || !e) return fail(RAOCP_ERR_ARG, "null argument");
    int rc = copy_in(c, c->cur_e, e, c->D, flags);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return RAOCP_OK;
}
int raocp_get_dual(raocp_ctx* c, double* e, int flags) {
    DevGuard dg_(c);
    if (!c || !e) return fail(RAOCP_ERR_ARG, "null argument");
    return copy_out(c, e, c->cur_e, c->D, flags);
}

// the cold start of Solver.chock on a fresh Cache: primal and dual zero on the device
int raocp_reset_iterate(raocp_ctx* c) {
    DevGuard dg_(c);
    if (!c) return fail(RAOCP_ERR_ARG, "null context");
    HIPCHK(hipMemsetAsync(c->cur_z, 0, c->P * c->wsz, c->stream));
    HIPCHK(hipMemsetAsync(c->cur_e, 0, c->D * c->wsz, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return RAOCP_OK;
}

int raocp_kernel_info(raocp_ctx* c, int op, char* buf, int cap) {
    DevGuard dg_(c);
    if (!c || !buf || cap < 1) return fail(RAOCP_ERR_ARG, "bad argument");
    const std::string s = kernel_name(c, op);
    if (s.empty() && op != 11 && op != 12 && op != 13 && op != 14 && op != 15 && op != 16 && op != 18 && op != 19 && op != 20) return fail(RAOCP_ERR_ARG, "unknown op " + std::to_string(op));
    snprintf(buf, (size_t)cap, "%s", s.c_str());
    return RAOCP_OK;
}

int raocp_set_initial_state(raocp_ctx* c, const double* x0) {
    DevGuard dg_(c);
    if (!c || !x0) return fail(RAOCP_ERR_ARG, "null argument");
    c->h_x0.assign(x0, x0 + c->nx);
    if (c->f32) {
        const std::vector<float> f(x0, x0 + c->nx);
        HIPCHK(hipMemcpy(c->x0, f.data(), c->nx * sizeof(float), hipMemcpyHostToDevice));
    } else {
        HIPCHK(hipMemcpy(c->x0, x0, c->nx * sizeof(double), hipMemcpyHostToDevice));
    }
    c->has_x0 = true;
    return RAOCP_OK;
}

int raocp_relax_s0(raocp_ctx* c, double alpha) {
    DevGuard dg_(c);
    if (c && c->f32) return fail(RAOCP_ERR_ARG, "not available on an fp32 context (the CP loop and L / L^T are)");
    if (!c) return fail(RAOCP_ERR_ARG, "null context");
    raocp::k_relax_s0<<<1, 1, 0, c->stream>>>(c->dev, c->cur_z, alpha);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return RAOCP_OK;
}

int raocp_project_on_dynamics(raocp_ctx* c) {
    DevGuard dg_(c);
    SweepLock sl_(c);
    if (c && c->f32 && !c->dyn32) return fail(RAOCP_ERR_ARG, "fp32 context without a dynamics plan");
    if (!c) return fail(RAOCP_ERR_ARG, "null context");
    if (!c->has_x0) return fail(RAOCP_ERR_STATE, "initial state not cached (call cache_initial_state first)");
    const raocp::Bufs solo{c->cur_z, c->cur_z, c->cur_z, c->cur_e, c->cur_e};
    launch_dynamics(c, solo, 0, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return fuse_err(c);
}

int raocp_project_on_kernel(raocp_ctx* c) {
    DevGuard dg_(c);
    if (c && c->f32) return fail(RAOCP_ERR_ARG, "not available on an fp32 context (the CP loop and L / L^T are)");
    if (!c) return fail(RAOCP_ERR_ARG, "null context");
    const Launch L = groups(c->cmax + 1, c->m);
    raocp::k_kernel_proj<<<L.blocks, kBlock, 0, c->stream>>>(c->dev, c->cur_z);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return RAOCP_OK;
}

int raocp_prox_f(raocp_ctx* c, double alpha) {
    DevGuard dg_(c);
    int rc;
    if ((rc = raocp_relax_s0(c, alpha)) || (rc = raocp_project_on_dynamics(c)) || (rc = raocp_project_on_kernel(c)))
        return rc;
    return RAOCP_OK;
}

int raocp_prox_gconj(raocp_ctx* c, double alpha) {
    DevGuard dg_(c);
    if (c && c->f32) return fail(RAOCP_ERR_ARG, "not available on an fp32 context (the CP loop and L / L^T are)");
    if (!c) return fail(RAOCP_ERR_ARG, "null context");
    int rc = set_ctl_alpha(c, alpha);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(&c->ctl->flags, 0, sizeof(int), c->stream));
    launch_cp_dual(c, false, c->cur_e);
    if (c->n_ph) raocp::k_zero_idx<<<cdiv(c->n_ph, kBlock), kBlock, 0, c->stream>>>(c->cur_e, c->ph, c->n_ph);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->h_ctl, c->ctl, sizeof(Ctl), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (int fe = fuse_err(c)) return fe;
    if (c->h_ctl->flags & 1) return fail(RAOCP_ERR_NAN_IN_BOX, "Rectangle constraint - 'nan' value cannot be constrained");
    return RAOCP_OK;
}

int raocp_dual_scale(raocp_ctx* c, double alpha) {
    DevGuard dg_(c);
    if (c && c->f32) return fail(RAOCP_ERR_ARG, "not available on an fp32 context (the CP loop and L / L^T are)");
    if (!c) return fail(RAOCP_ERR_ARG, "null context");
    raocp::k_div<<<std::min(2048, cdiv((int)c->D, kBlock)), kBlock, 0, c->stream>>>(c->cur_e, alpha, (int)c->D);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return RAOCP_OK;
}

int raocp_dual_add_halves(raocp_ctx* c) {
    DevGuard dg_(c);
    if (c && c->f32) return fail(RAOCP_ERR_ARG, "not available on an fp32 context (the CP loop and L / L^T are)");
    if (!c) return fail(RAOCP_ERR_ARG, "null context");
    const Dev& D = c->dev;
    const int nb = cdiv(c->n, kBlock);
    raocp::k_add_const<<<nb, kBlock, 0, c->stream>>>(c->cur_e, -0.5, D.E5, D.E6);
    raocp::k_add_const<<<nb, kBlock, 0, c->stream>>>(c->cur_e, 0.5, D.E6, D.E7);
    raocp::k_add_const<<<nb, kBlock, 0, c->stream>>>(c->cur_e, -0.5, D.E12, D.E13);
    raocp::k_add_const<<<nb, kBlock, 0, c->stream>>>(c->cur_e, 0.5, D.E13, D.E14);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return RAOCP_OK;
}

int raocp_dual_project(raocp_ctx* c, int which) {
    DevGuard dg_(c);
    if (c && c->f32) return fail(RAOCP_ERR_ARG, "not available on an fp32 context (the CP loop and L / L^T are)");
    if (!c) return fail(RAOCP_ERR_ARG, "null context");
    HIPCHK(hipMemsetAsync(&c->ctl->flags, 0, sizeof(int), c->stream));
    const int mode = (which & 1 ? raocp::kDualNonleaf : 0) | (which & 2 ? raocp::kDualLeaf : 0);
    launch_cp_dual(c, false, c->cur_e, mode);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->h_ctl, c->ctl, sizeof(Ctl), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (int fe = fuse_err(c)) return fe;
    if (c->h_ctl->flags & 1) return fail(RAOCP_ERR_NAN_IN_BOX, "Rectangle constraint - 'nan' value cannot be constrained");
    return RAOCP_OK;
}

int raocp_dual_moreau(raocp_ctx* c, double alpha, const double* modified) {
    DevGuard dg_(c);
    if (c && c->f32) return fail(RAOCP_ERR_ARG, "not available on an fp32 context (the CP loop and L / L^T are)");
    if (!c || !modified) return fail(RAOCP_ERR_ARG, "null argument");
    int rc = copy_in(c, c->tmpD, modified, c->D, 0);
    if (rc) return rc;
    raocp::k_moreau<<<std::min(2048, cdiv((int)c->D, kBlock)), kBlock, 0, c->stream>>>(c->cur_e, c->tmpD, alpha,
                                                                                        (int)c->D);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return RAOCP_OK;
}

// ---- step size: Lanczos on L'L with device mat-vecs (replaces ARPACK, solver.py:109-118)
static double tridiag_max_eig(const std::vector<double>& a, const std::vector<double>& b) {
    // largest eigenvalue of the symmetric tridiagonal (a diag, b off-diag) by Sturm bisection
    const int k = (int)a.size();
    double lo = a[0], hi = a[0];
    for (int i = 0; i < k; ++i) {
        const double r = (i > 0 ? std::fabs(b[i - 1]) : 0.0) + (i + 1 < k ? std::fabs(b[i]) : 0.0);
        lo = std::min(lo, a[i] - r);
        hi = std::max(hi, a[i] + r);
    }
    auto count_greater = [&](double x) {
        int cnt = 0;
        double dd = 1.0;
        for (int i = 0; i < k; ++i) {
            const double bb = i > 0 ? b[i - 1] * b[i - 1] : 0.0;
            dd = (a[i] - x) - (i > 0 ? bb / dd : 0.0);
            if (dd == 0.0) dd = -1e-300;
            if (dd > 0) ++cnt;
        }
        return cnt;  // number of eigenvalues > x
    };
    for (int it = 0; it < 200 && hi - lo > 1e-16 * std::max(1.0, std::fabs(hi)); ++it) {
        const double mid = 0.5 * (lo + hi);
        if (count_greater(mid) >= 1) lo = mid;
        else hi = mid;
    }
    return 0.5 * (lo + hi);
}

static int dev_dot(raocp_ctx* c, const double* a, const double* b, int n, double* out) {
    const int nb = std::min(1024, cdiv(n, kBlock));
    if (c->f32) raocp::k_dot_partial<float><<<nb, kBlock, 0, c->stream>>>((const float*)a, (const float*)b, n, c->part);
    else raocp::k_dot_partial<double><<<nb, kBlock, 0, c->stream>>>(a, b, n, c->part);
    raocp::k_dot_final<<<1, kBlock, 0, c->stream>>>(c->part, nb, c->scal);
    HIPCHK(hipMemcpyAsync(out, c->scal, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return RAOCP_OK;
}

static void dev_scale_copy(raocp_ctx* c, int nb, double sc, const double* x, double* y, int n) {
    if (c->f32) raocp::k_scale_copy<float><<<nb, kBlock, 0, c->stream>>>(sc, (const float*)x, (float*)y, n);
    else raocp::k_scale_copy<double><<<nb, kBlock, 0, c->stream>>>(sc, x, y, n);
}
static void dev_axpby(raocp_ctx* c, int nb, double a, const double* x, double b, double* y, int n) {
    if (c->f32) raocp::k_axpby<float><<<nb, kBlock, 0, c->stream>>>(a, (const float*)x, b, (float*)y, n);
    else raocp::k_axpby<double><<<nb, kBlock, 0, c->stream>>>(a, x, b, y, n);
}

int raocp_step_size(raocp_ctx* c, double* lambda_max, int max_it, double rtol) {
    DevGuard dg_(c);
    if (!c || !lambda_max) return fail(RAOCP_ERR_ARG, "null argument");
    if (int ra = ell_available(c)) return ra;
    if (max_it <= 0) max_it = 300;
    if (rtol <= 0) rtol = 1e-14;
    const int P = (int)c->P;
    max_it = std::min<int64_t>(max_it, c->P);
    double *v = nullptr, *vprev = nullptr, *w = nullptr, *eta = nullptr;
    int rc;
    if ((rc = c->alloc(&v, P)) || (rc = c->alloc(&vprev, P)) || (rc = c->alloc(&w, P)) || (rc = c->alloc(&eta, c->D)))
        return rc;
    std::vector<double> h(P);
    std::mt19937_64 gen(12345);
    std::normal_distribution<double> nd(0.0, 1.0);
    for (int i = 0; i < P; ++i) h[i] = nd(gen);
    h[c->dev.T0] = 0.0;  // tau_0 is outside the range of L'L (the reference's template keeps it 0)
    if ((rc = copy_in(c, v, h.data(), P, 0))) return rc;
    HIPCHK(hipMemsetAsync(vprev, 0, P * sizeof(double), c->stream));
    HIPCHK(hipMemsetAsync(w, 0, P * sizeof(double), c->stream));
    HIPCHK(hipMemsetAsync(eta, 0, c->D * sizeof(double), c->stream));
    const int nbv = std::min(2048, cdiv(P, kBlock));
    double nrm2;
    if ((rc = dev_dot(c, v, v, P, &nrm2))) return rc;
    dev_scale_copy(c, nbv, 1.0 / std::sqrt(nrm2), v, v, P);
    std::vector<double> al, be;
    double beta = 0.0, lam = 0.0, lam_prev = -1.0;
    int stable = 0;
    for (int j = 0; j < max_it; ++j) {
        launch_ell(c, v, eta);
        HIPCHK(hipMemsetAsync(w, 0, P * sizeof(double), c->stream));
        launch_ell_t(c, eta, w);          // w = L'L v (tau_0 = 0)
        dev_axpby(c, nbv, -beta, vprev, 1.0, w, P);
        double a;
        if ((rc = dev_dot(c, w, v, P, &a))) return rc;
        dev_axpby(c, nbv, -a, v, 1.0, w, P);
        double bb;
        if ((rc = dev_dot(c, w, w, P, &bb))) return rc;
        al.push_back(a);
        lam = tridiag_max_eig(al, be);
        beta = std::sqrt(bb);
        if (std::fabs(lam - lam_prev) <= rtol * std::fabs(lam)) {
            if (++stable >= 3) break;
        } else {
            stable = 0;
        }
        lam_prev = lam;
        if (beta <= 1e-300) break;
        be.push_back(beta);
        // vprev <- v ; v <- w / beta
        HIPCHK(hipMemcpyAsync(vprev, v, P * c->wsz, hipMemcpyDeviceToDevice, c->stream));
        dev_scale_copy(c, nbv, 1.0 / beta, w, v, P);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    for (double* p : {v, vprev, w, eta}) {
        (void)hipFree(p);
        c->allocs.erase(std::remove(c->allocs.begin(), c->allocs.end(), (void*)p), c->allocs.end());
    }
    *lambda_max = lam;
    return RAOCP_OK;
}

int raocp_cp_run(raocp_ctx* c, const double* x0, int max_iters, double tol, double alpha, int* status, int* iters,
                 double* err_hist, double* delta_hist) {
    DevGuard dg_(c);
    SweepLock sl_(c);
    if (c && c->f32 && !c->dyn32) return fail(RAOCP_ERR_ARG, "fp32 CP loop unavailable: no fp32 dynamics plan");
    if (!c || !x0) return fail(RAOCP_ERR_ARG, "null argument");
    if (max_iters < 0) return fail(RAOCP_ERR_ARG, "max_iters must be >= 0");
    int rc;
    if ((rc = ensure_hist(c, (size_t)max_iters + 1))) return rc;
    if ((rc = raocp_set_initial_state(c, x0))) return rc;
    if ((rc = cp_init(c, x0, max_iters, tol, alpha, true))) return rc;
    {
        const int batch = kGraphBatch;
        if ((rc = ensure_graph(c, batch))) return rc;
        const bool pub = defer_check(c);
        for (;;) {
            if (pub) c->h_pub->ctl.final_k = -2;
            if ((rc = launch_batch(c, batch))) return rc;
            if (!pub) HIPCHK(hipMemcpyAsync(c->h_ctl, c->ctl, sizeof(Ctl), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            if (pub) *c->h_ctl = c->h_pub->ctl;  // published by the batch's last stopping test
            if (c->h_ctl->done) break;
        }
    }
    const int fk = c->h_ctl->final_k;
    if (int rh = copy_hist(c, fk, err_hist, delta_hist)) return rh;
    c->cur_z = c->Z[(fk + 1) % 3];
    c->cur_e = c->E[(fk + 1) % 2];
    if (iters) *iters = fk + 1;
    if (status) *status = fk < max_iters ? 0 : 1;
    if (int fe = fuse_err(c)) return fe;
    if (c->h_ctl->flags & 1) return fail(RAOCP_ERR_NAN_IN_BOX, "Rectangle constraint - 'nan' value cannot be constrained");
    return RAOCP_OK;
}

int raocp_cp_prepare(raocp_ctx* c, const double* x0, int iters, double alpha) {
    DevGuard dg_(c);
    if (c && c->f32 && !c->dyn32) return fail(RAOCP_ERR_ARG, "fp32 CP loop unavailable: no fp32 dynamics plan");
    if (!c || iters < 1) return fail(RAOCP_ERR_ARG, "bad argument");
    int rc;
    if ((rc = ensure_hist(c, (size_t)iters + 1))) return rc;
    if (iters / kGraphBatch && (rc = ensure_graph(c, kGraphBatch))) return rc;
    if (iters % kGraphBatch && (rc = ensure_graph(c, iters % kGraphBatch))) return rc;
    if (x0) {
        // one dry replay of each graph the run launches, with ctl->done set (every kernel leaves
        // without arithmetic): the graphs' first-launch cost (measured ~20 us at K = 20 beyond
        // hipGraphUpload, tools/k_sweep.py) falls here instead of in the timed call
        if (!c->eager) {
            HIPCHK(hipStreamSynchronize(c->stream));
            Ctl h{};
            h.done = 1;
            h.final_k = -1;
            *c->h_ctl = h;
            HIPCHK(hipMemcpyAsync(c->ctl, c->h_ctl, sizeof(Ctl), hipMemcpyHostToDevice, c->stream));
            if (iters / kGraphBatch && (rc = launch_batch(c, kGraphBatch))) return rc;
            if (iters % kGraphBatch && (rc = launch_batch(c, iters % kGraphBatch))) return rc;
            HIPCHK(hipStreamSynchronize(c->stream));
            if (int fe = fuse_err(c)) return fe;
        }
        // the run's initial state: the following raocp_cp_bench(ctx, NULL, iters, ...) starts here
        if ((rc = cp_init(c, x0, iters - 1, 0.0, alpha))) return rc;
        HIPCHK(hipStreamSynchronize(c->stream));
        c->prepared = iters;
    }
    return RAOCP_OK;
}

int raocp_cp_bench(raocp_ctx* c, const double* x0, int iters, double alpha, float* ms) {
    DevGuard dg_(c);
    SweepLock sl_(c);
    if (c && c->f32 && !c->dyn32) return fail(RAOCP_ERR_ARG, "fp32 CP loop unavailable: no fp32 dynamics plan");
    if (!c || iters < 1) return fail(RAOCP_ERR_ARG, "bad argument");
    int rc;
    if ((rc = ensure_hist(c, (size_t)iters + 1))) return rc;
    const int batch = kGraphBatch, full = iters / batch, rem = iters % batch;
    if (full && (rc = ensure_graph(c, batch))) return rc;
    if (rem && (rc = ensure_graph(c, rem))) return rc;
    if (x0) {
        if ((rc = cp_init(c, x0, iters - 1, 0.0, alpha))) return rc;
    } else if (c->prepared != iters) {
        return fail(RAOCP_ERR_STATE, "raocp_cp_bench without x0 needs raocp_cp_prepare(ctx, x0, iters, alpha) first");
    }
    c->prepared = 0;
    if (!c->ev0) {
        HIPCHK(hipEventCreate(&c->ev0));
        HIPCHK(hipEventCreate(&c->ev1));
    }
    hipEvent_t e0 = c->ev0, e1 = c->ev1;
    if (x0) HIPCHK(hipStreamSynchronize(c->stream));
    // the batch tail's stopping test publishes the control block and the error word to pinned
    // host memory (k_cp_check pub): no device-to-host copy behind the timed kernels
    const bool pub = defer_check(c);
    raocp::CtlPub* hp = c->h_pub;
    if (pub) hp->ctl.final_k = -2;
    HIPCHK(hipEventRecord(e0, c->stream));
    // exactly `iters` iterations' kernels: whole batches, then the remainder batch (an RCCL
    // shard then runs the last iteration's deferred stopping test)
    for (int b = 0; b < full; ++b)
        if ((rc = launch_batch(c, batch))) return rc;
    if (rem && (rc = launch_batch(c, rem))) return rc;
    if (c->comm && (rc = enqueue_shard_tail(c))) return rc;
    HIPCHK(hipEventRecord(e1, c->stream));
    const unsigned* ew = err_word(c);
    if (!pub) {
        HIPCHK(hipMemcpyAsync(&hp->ctl, c->ctl, sizeof(Ctl), hipMemcpyDeviceToHost, c->stream));
        hp->err = 0;
        if (ew) HIPCHK(hipMemcpyAsync(&hp->err, ew, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipEventElapsedTime(ms, e0, e1));
    *c->h_ctl = hp->ctl;
    if (ew && hp->err)
        if (int fe = fuse_err(c)) return fe;  // a timed-out hand-off skipped its arithmetic
    if (c->h_ctl->final_k != iters - 1) return fail(RAOCP_ERR_STATE, "bench did not run the requested iterations");
    c->cur_z = c->Z[iters % 3];
    c->cur_e = c->E[iters % 2];
    return RAOCP_OK;
}

// diagnostics: run the dynamics projection once on the current primal with in-kernel
// stamps enabled (k_dyn_top: prologue, each backward / forward stage); returns up to
// `cap` raw 100 MHz timestamps.
int raocp_debug_dyn_stamps(raocp_ctx* c, unsigned long long* out, int cap) {
    DevGuard dg_(c);
    SweepLock sl_(c);
    // the regular-tree sweeps' stamps need only their own unit built with them (VAR_UNIT=dynr)
    const bool dr = c && c->path.dyn == DynPath::Dr;
    if (!raocp::kDiag && !(dr && raocp::dr_diag_build()))
        return fail(RAOCP_ERR_ARG, "in-kernel stamps need a diagnostic build (make DIAG=1)");
    if (c && c->f32) return fail(RAOCP_ERR_ARG, "not available on an fp32 context (the CP loop and L / L^T are)");
    if (!c || !out || cap <= 0) return fail(RAOCP_ERR_ARG, "bad argument");
    // k_dr / k_drc stamp 4 slots per workgroup from slot 1024 (raocp_dynr.hip wg_stamp) and
    // k_drc's CP waves 128 slots from 3072
    if (dr && (size_t)cap < std::max(c->path.fused ? (size_t)3072 + 128 : (size_t)0, 1024 + 4 * ((size_t)c->drp.nblk + 1)))
        return fail(RAOCP_ERR_ARG, "stamp buffer too small for the regular-tree sweep's workgroup stamps");
    // the tiered sweep stamps 64 slots per launch (2 per tier + the top)
    if (c->cut > 0 && (size_t)cap < 64 * (2 * c->tiers.size() + 1))
        return fail(RAOCP_ERR_ARG, "stamp buffer too small: 64 slots per dynamics launch");
    unsigned long long* st = nullptr;
    int rc = c->alloc(&st, (size_t)cap);
    if (rc) return rc;
    HIPCHK(hipMemset(st, 0, cap * sizeof(unsigned long long)));
    Dev saved = c->dev;
    c->dev.stamps = st;
    const raocp::Bufs solo{c->cur_z, c->cur_z, c->cur_z, c->cur_e, c->cur_e};
    // RAOCP_STAMP_KERNEL: the launch to stamp (its first letter) and, for the CP kernels, the
    // workgroup / task that records (the number after it, e.g. "c200")
    const char* which = getenv("RAOCP_STAMP_KERNEL");
    if (which && which[0]) c->dev.cp_dbg = atoi(which + 1);
    const char w = which ? which[0] : 0;
    if (w == 'c' && !raocp::cp_fused(c->path.cp)) return fail(RAOCP_ERR_ARG, "no fused CP kernel on this context");
    if (w == 'f' && !c->path.fused) return fail(RAOCP_ERR_ARG, "no fused dynamics + CP launch on this context");
    if (w == 'p' || w == 'c' || w == 'f') {  // the CP kernels run on a valid control block
        std::vector<double> x0(c->nx, 0.0);
        int rc2 = cp_init(c, x0.data(), 1 << 30, 0.0, 0.5);
        if (rc2) return rc2;
    }
    if (w == 'p') {  // k_cpp (diagnostics)
        launch_cpp(c);
    } else if (w == 'c') {  // the fused CP kernel (k_cp6 / k_cp5 / k_cp4 / k_cp3)
        launch_cp_fused(c);
    } else if (w == 'f') {  // the fused dynamics + CP launch (k_drc)
        const raocp::Bufs keep = c->bufs;
        c->bufs = rotated(c, 0);
        launch_drc(c, 0, false);
        c->bufs = keep;
    } else if (w == 'l') {  // k_ell on the staging buffers
        launch_ell(c, c->tmpP, c->tmpD);
    } else if (w == 't') {  // k_ell_t
        launch_ell_t(c, c->tmpD, c->tmpP);
    } else {
        launch_dynamics(c, solo, 0, nullptr);
    }
    c->dev = saved;
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(out, st, cap * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return RAOCP_OK;
}


// ---- subtree sharding ---------------------------------------------------------------
int raocp_shard_setup(raocp_ctx* c, int nranks, int rank) {
    DevGuard dg_(c);
    const bool dyn3 = c && c->path.dyn == DynPath::Dyn3;  // k_dy3 is a context's sweep sharded or not
    if (c && c->f32 && !dyn3)
        return fail(RAOCP_ERR_ARG, "fp32 sharding needs the per-stage streaming dynamics (uniform branching and slots)");
    if (!c || nranks < 1 || rank < 0 || rank >= nranks) return fail(RAOCP_ERR_ARG, "bad shard arguments");
    // one shard is the unsharded solve, unless forced (tests run the exchange path with R = 1)
    if (nranks == 1 && !getenv("RAOCP_SHARD_FORCE")) return RAOCP_OK;
    const int N = c->N;
    int S = c->cut;
    if (dyn3) {
        // the per-stage sweep: cut at the first stage with at least 8 subtrees per shard (the
        // replicated top above it is a few hundred nodes at most)
        S = 0;
        for (int t = 1; t < N && !S; ++t)
            if (c->stage_ptr[t + 1] - c->stage_ptr[t] >= 8 * nranks) S = t;
        if (!S) return fail(RAOCP_ERR_ARG, "tree too small to shard (no stage with 8 subtrees per shard)");
    } else if (S <= 0 || S >= N || c->tiers.empty()) {
        return fail(RAOCP_ERR_ARG, "tree too small to shard (the dynamics plan has no tier below the top)");
    }
    const int nb = c->stage_ptr[S + 1] - c->stage_ptr[S];
    if (nb < nranks) return fail(RAOCP_ERR_ARG, "fewer subtrees at the cut stage than shards");
    c->sh_R = nranks;
    c->sh_r = rank;
    c->sh_S = S;
    std::vector<int> slc(2 * nranks);
    int xmax = 0;
    for (int r = 0; r < nranks; ++r) {
        const int lo = c->stage_ptr[S] + (int)((long)r * nb / nranks), hi = c->stage_ptr[S] + (int)((long)(r + 1) * nb / nranks);
        slc[2 * r] = lo;
        slc[2 * r + 1] = hi - lo;
        xmax = std::max(xmax, hi - lo);
    }
    c->x_max = xmax;
    c->own_first = slc[2 * rank];
    c->own_cnt = slc[2 * rank + 1];
    // owned id range per stage: the whole stage above the cut, descendants below
    c->own_lo.assign(N + 1, 0);
    c->own_hi.assign(N + 1, 0);
    for (int t = 0; t < S; ++t) {
        c->own_lo[t] = c->stage_ptr[t];
        c->own_hi[t] = c->stage_ptr[t + 1];
    }
    int lo = c->own_first, hi = c->own_first + c->own_cnt;
    for (int t = S; t <= N; ++t) {
        c->own_lo[t] = lo;
        c->own_hi[t] = hi;
        if (t < N && hi > lo) {
            const int nlo = c->h_chs[lo], nhi = c->h_chs[hi - 1] + c->h_nch[hi - 1];
            lo = nlo;
            hi = nhi;
        }
    }
    c->tier_own.clear();
    if (!dyn3)
        for (const auto& tp : c->tiers)
            c->tier_own.push_back({c->own_lo[tp.s0] - c->stage_ptr[tp.s0], c->own_hi[tp.s0] - c->own_lo[tp.s0]});
    c->d3own = c->d3st;
    for (int t = S; t < N && dyn3; ++t) {
        c->d3own[t].i0 = c->own_lo[t];
        c->d3own[t].i1 = c->own_hi[t];
    }
    // CP blocks: the replicated top families plus the owned ones, the owned leaves
    std::vector<std::pair<int, int>> pr_;
    pr_.push_back({0, c->stage_ptr[S]});
    for (int t = S; t < N; ++t)
        if (c->own_hi[t] > c->own_lo[t]) pr_.push_back({c->own_lo[t], c->own_hi[t]});
    std::vector<std::pair<int, int>> lr_{{c->own_lo[N], c->own_hi[N]}};
    int rc;
    if ((rc = build_cp_blocks(c, pr_, lr_))) return rc;
    // the fused forms' task lists (for every form that was set up). The first launch's parent ranges: the
    // owned leaf parents, the owned families above them and the replicated top above the cut's parents
    std::vector<std::pair<int, int>> ra;
    if (N - 1 >= S) ra.push_back({c->own_lo[N - 1], c->own_hi[N - 1]});
    for (int t = S; t < N - 1; ++t) ra.push_back({c->own_lo[t], c->own_hi[t]});
    if (S >= 2) ra.push_back({0, c->stage_ptr[S - 1]});
    if (c->cp3) {
        // k_cp3 in two launches: the owned families and leaves plus the replicated top above
        // the cut's parents (storing its roots' xi2 for X1), then the cut's parents with the
        // roots' eta2 entries from X1
        const long ta = cp3_tasks(c->cp3_ta, ra, c->own_lo[N], c->cp3_split ? c->own_hi[N] : c->own_lo[N], c->cp3_split,
                                  c->cp3_mL);
        c->cp3_ta.xlo = c->own_first;
        c->cp3_ta.xhi = c->own_first + c->own_cnt;
        const long tb = cp3_tasks(c->cp3_tb, {{c->stage_ptr[S - 1], c->stage_ptr[S]}}, 0, 0, c->cp3_split, c->cp3_mL);
        if (ta < 0 || tb < 0)
            return fail(RAOCP_ERR_ARG, "shard's k_cp3 task list exceeds its " + std::to_string(raocp::kCp3MaxR) +
                                           " parent-range slots (too many stages below the cut)");
        c->cp3_tb.ext2 = 1;
        c->cp3_grid = cp3_grid_of(ta);
        c->cp3_gridb = cp3_grid_of(tb);
        c->cp_rows = c->cp3_grid + c->cp3_gridb;
        if ((rc = ensure_red_rows(c, c->cp_rows))) return rc;
        HIPCHK(hipMemset(c->redpart, 0, (size_t)c->red_rows * 6 * sizeof(double)));
    }
    if (c->cp5) {
        // k_cp5 in two launch pairs: the eta2 tasks of the replicated top and the owned stages,
        // the owned leaves, and the owned families plus the top above the cut's parents; after
        // X1 (the roots' s of the half step) the cut's parents' family tiles alone
        std::vector<std::pair<int, int>> er{{0, c->stage_ptr[S]}};
        for (int t = S; t < N; ++t) er.push_back({c->own_lo[t], c->own_hi[t]});
        if (cp3_tasks(c->cp5_et, er, 0, 0, 1, 0, 64) < 0 || cp3_tasks(c->cp5_tk, ra, 0, 0, 1, c->cp3_mL) < 0 ||
            cp3_tasks(c->cp5_tkb, {{c->stage_ptr[S - 1], c->stage_ptr[S]}}, 0, 0, 1, c->cp3_mL) < 0)
            return fail(RAOCP_ERR_ARG, "shard's k_cp5 task lists exceed their " + std::to_string(raocp::kCp3MaxR) +
                                           " range slots (too many stages below the cut)");
        c->cp5_gl = raocp::cp5_leaf_grid(c->cp5_et, c->own_lo[N], c->own_hi[N], c->cp5_lpf);
        c->cp5_gf = raocp::cp5_fam_grid(c->cp5_tk);
        c->cp5_gfb = raocp::cp5_fam_grid(c->cp5_tkb);
        c->cp_rows = raocp::cp5_rows(c->cp5_gl, c->cp5_gf) + c->cp5_gfb;
        if ((rc = ensure_red_rows(c, c->cp_rows))) return rc;
        HIPCHK(hipMemset(c->redpart, 0, (size_t)c->red_rows * 6 * sizeof(double)));
    }
    if ((rc = c->alloc(&c->x2_send, (size_t)xmax * std::max(c->KP, c->nx))) ||
        (rc = c->alloc(&c->x2_recv, (size_t)nranks * xmax * std::max(c->KP, c->nx))) ||
        (rc = c->alloc(&c->x1_send, (size_t)2 * xmax + 16)) || (rc = c->alloc(&c->x1_recv, (size_t)nranks * (2 * xmax + 16))) ||
        (rc = c->alloc(&c->red8, 16)) || (rc = c->upload_vec(&c->d_slc, slc)))
        return rc;
    resolve_ctx_paths(c);  // sh_S > 0 now: the whole-tree forms are off
    drop_graphs(c);
    return RAOCP_OK;
}

int raocp_shard_owned(raocp_ctx* c, int32_t* lo, int32_t* hi, int cap) {
    DevGuard dg_(c);
    if (!c || !lo || !hi) return fail(RAOCP_ERR_ARG, "null argument");
    for (int t = 0; t <= c->N && t < cap; ++t) {
        lo[t] = c->sh_S > 0 ? c->own_lo[t] : c->stage_ptr[t];
        hi[t] = c->sh_S > 0 ? c->own_hi[t] : c->stage_ptr[t + 1];
    }
    return RAOCP_OK;
}

int raocp_comm_unique_id(unsigned char* out128) {
    if (!out128) return fail(RAOCP_ERR_ARG, "null argument");
    int rc;
    if ((rc = rccl_load())) return rc;
    ncclUniqueId id;
    if ((rc = rccl_check(g_rccl.get_id(&id), "ncclGetUniqueId"))) return rc;
    memcpy(out128, id.internal, NCCL_UNIQUE_ID_BYTES);
    return RAOCP_OK;
}

int raocp_comm_init(raocp_ctx* c, const unsigned char* id128, int nranks, int rank) {
    DevGuard dg_(c);
    if (!c || !id128) return fail(RAOCP_ERR_ARG, "null argument");
    if (c->sh_R != nranks || c->sh_r != rank) return fail(RAOCP_ERR_STATE, "call raocp_shard_setup with the same ranks first");
    int rc;
    if ((rc = rccl_load())) return rc;
    HIPCHK(hipSetDevice(c->device));
    ncclUniqueId id;
    memcpy(id.internal, id128, NCCL_UNIQUE_ID_BYTES);
    ncclComm_t comm = nullptr;
    if ((rc = rccl_check(g_rccl.init_rank(&comm, nranks, id, rank), "ncclCommInitRank"))) return rc;
    c->comm = comm;
    drop_graphs(c);
    return RAOCP_OK;
}

// Shards that share one process and one device (tests, and a host-driven transport):
// the CP loop runs eagerly, the exchanges are device copies between the shards' buffers.
// warm: every shard starts from its own current primal / dual (raocp_set_primal / raocp_set_dual,
// or the end of its last run), as raocp_cp_run does; the entries a shard does not own are whatever
// it holds and stay so.
int raocp_group_cp_run_warm(raocp_ctx** cs, int R, const double* x0, int max_iters, double tol, double alpha, int warm,
                            int* status, int* iters, double* err_hist, double* delta_hist) {
    if (!cs || R < 1 || !x0) return fail(RAOCP_ERR_ARG, "null argument");
    DevGuard dg_(cs[0]);
    for (int r = 0; r < R; ++r)
        if (!cs[r] || cs[r]->sh_R != R || cs[r]->sh_r != r) return fail(RAOCP_ERR_STATE, "shards not set up for this group");
    int rc;
    for (int r = 0; r < R; ++r) {
        raocp_ctx* c = cs[r];
        HIPCHK(hipSetDevice(c->device));
        if ((rc = ensure_hist(c, (size_t)max_iters + 1))) return rc;
        if ((rc = raocp_set_initial_state(c, x0))) return rc;
        if ((rc = cp_init(c, x0, max_iters, tol, alpha, warm != 0))) return rc;
    }
    auto sync_all = [&]() -> int {
        for (int r = 0; r < R; ++r) HIPCHK(hipStreamSynchronize(cs[r]->stream));
        return RAOCP_OK;
    };
    // the RCCL iteration's protocol with device copies as the transport: X2 after the tiers'
    // backward sweeps, X1 (roots' eta2 entries + the previous iteration's residual record,
    // whose stopping test runs on arrival) after k_cpd; the loop ends once the (deferred)
    // test has fired
    for (int k = 0;; ++k) {
        for (int r = 0; r < R; ++r) {
            raocp_ctx* c = cs[r];
            c->bufs = rotated(c, k % 6);
            shard_phase_back(c);
        }
        if ((rc = sync_all())) return rc;
        for (int r = 0; r < R; ++r) {
            raocp_ctx* c = cs[r];
            for (int q = 0; q < R; ++q)
                HIPCHK(hipMemcpyAsync((char*)c->x2_recv + (size_t)q * x2_bytes(c), cs[q]->x2_send, x2_bytes(c),
                                      hipMemcpyDeviceToDevice, c->stream));
            shard_phase_fwd(c);
        }
        if ((rc = sync_all())) return rc;
        for (int r = 0; r < R; ++r) {
            raocp_ctx* c = cs[r];
            for (int q = 0; q < R; ++q)
                HIPCHK(hipMemcpyAsync(c->x1_recv + (size_t)q * x1_len(c), cs[q]->x1_send, (size_t)x1_len(c) * sizeof(double),
                                      hipMemcpyDeviceToDevice, c->stream));
            shard_phase_top(c);
            HIPCHK(hipMemcpyAsync(c->h_ctl, c->ctl, sizeof(Ctl), hipMemcpyDeviceToHost, c->stream));
        }
        if ((rc = sync_all())) return rc;
        HIPCHK(hipGetLastError());
        if (cs[0]->h_ctl->done) break;
    }
    for (int r = 0; r < R; ++r) cs[r]->bufs = raocp::Bufs{cs[r]->Z[0], cs[r]->Z[1], cs[r]->Z[2], cs[r]->E[0], cs[r]->E[1]};
    raocp_ctx* c = cs[0];
    const int fk = c->h_ctl->final_k;
    if (int rh = copy_hist(c, fk, err_hist, delta_hist)) return rh;
    for (int r = 0; r < R; ++r) {
        cs[r]->cur_z = cs[r]->Z[(fk + 1) % 3];
        cs[r]->cur_e = cs[r]->E[(fk + 1) % 2];
    }
    if (iters) *iters = fk + 1;
    if (status) *status = fk < max_iters ? 0 : 1;
    if (int fe = fuse_err(c)) return fe;
    if (c->h_ctl->flags & 1) return fail(RAOCP_ERR_NAN_IN_BOX, "Rectangle constraint - 'nan' value cannot be constrained");
    return RAOCP_OK;
}

int raocp_group_cp_run(raocp_ctx** cs, int R, const double* x0, int max_iters, double tol, double alpha, int* status,
                       int* iters, double* err_hist, double* delta_hist) {
    return raocp_group_cp_run_warm(cs, R, x0, max_iters, tol, alpha, 0, status, iters, err_hist, delta_hist);
}

int raocp_op_bench(raocp_ctx* c, int op, int reps, float* ms_per_launch) {
    DevGuard dg_(c);
    SweepLock sl_(c);
    if (!c || reps < 1 || !ms_per_launch) return fail(RAOCP_ERR_ARG, "bad argument");
    if (op == 17) {
        // the launches of one raocp_evaluate on the context's current primal, reps times, between two
        // events; nothing of the context moves (no random inputs, no control block)
        if (c->comm || c->sh_R != 1) return fail(RAOCP_ERR_STATE, "the evaluation is not available on a sharded context");
        if (!c->has_x0) return fail(RAOCP_ERR_STATE, "no initial state has been set");
        if (int re = eval_ensure(c)) return re;
        const raocp::EvalArg a = eval_arg(c, c->cur_z, c->x0);
        HIPCHK(raocp::eval_launch(c->dev, a, c->eval_plan, c->f32, c->stream));  // warm-up
        hipEvent_t e0, e1;
        HIPCHK(hipEventCreate(&e0));
        HIPCHK(hipEventCreate(&e1));
        HIPCHK(hipEventRecord(e0, c->stream));
        for (int i = 0; i < reps; ++i) HIPCHK(raocp::eval_launch(c->dev, a, c->eval_plan, c->f32, c->stream));
        HIPCHK(hipEventRecord(e1, c->stream));
        HIPCHK(hipEventSynchronize(e1));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        *ms_per_launch = ms / reps;
        return RAOCP_OK;
    }
    if (op == 0 || op == 1)
        if (int ra = ell_available(c)) return ra;
    // random inputs (seed 1), resident in HBM
    if (int rci = bench_inputs(c)) return rci;
    HIPCHK(hipStreamSynchronize(c->stream));
    double* outP = c->Z[2];
    double* outD = c->E[1];
    // ops >= 2 time the CP kernels (or one role of them) on a valid control block
    if (op >= 2) {
        if (c->f32 && (!c->dyn32 || (op != 2 && op != 6 && op != 9 && op != 10)))
            return fail(RAOCP_ERR_ARG, "fp32 context: ops 0, 1, 2, 6, 9 and 10 can be timed");
        if (int rh = ensure_hist(c, (size_t)reps + 16)) return rh;
        std::vector<double> x0(c->nx, 0.0);
        int rc = cp_init(c, x0.data(), 1 << 30, 0.0, 0.5);
        if (rc) return rc;
        for (int b = 0; b < 3; ++b) HIPCHK(hipMemcpyAsync(c->Z[b], c->tmpP, c->P * c->wsz, hipMemcpyDeviceToDevice, c->stream));
        for (int b = 0; b < 2; ++b) HIPCHK(hipMemcpyAsync(c->E[b], c->tmpD, c->D * c->wsz, hipMemcpyDeviceToDevice, c->stream));
    }
    auto run = [&]() {
        switch (op) {
            case 0: launch_ell(c, c->tmpP, outD); break;
            case 1: launch_ell_t(c, c->tmpD, outP); break;
            case 2: launch_cpd(c); break;
            case 3: case 4: case 5: launch_cp_dual(c, true, nullptr, raocp::kDualAll, op - 2); break;
            case 6: launch_cpp(c); break;
            case 7: case 8: launch_cp_primal(c, true, op - 6); break;
            case 9: launch_dynamics(c, c->bufs, 1, c->ctl); break;
            case 10: launch_cp_after_sweep(c); break;  // the CP iteration's kernels after the dynamics
            case 11: launch_drc(c, 0, false); break;  // the fused dynamics + CP launch (k_drc)
            default: raocp::k_cp_check<<<1, kBlock, 0, c->stream>>>(c->ctl, c->hist, c->redpart, c->cp_rows, 0, nullptr, nullptr);
        }
    };
    for (int i = 0; i < 3; ++i) run();  // warm-up
    // the reps launches replay as one graph (as in the CP loop), so the time is the
    // kernels' back to back, not the host's launch rate; RAOCP_EAGER=1 launches them
    // one by one (rocprofv3 kernel tracing)
    hipGraphExec_t gx = nullptr;
    if (!c->eager) {
        hipGraph_t g = nullptr;
        HIPCHK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
        for (int i = 0; i < reps; ++i) run();
        HIPCHK(hipStreamEndCapture(c->stream, &g));
        HIPCHK(hipGraphInstantiate(&gx, g, nullptr, nullptr, 0));
        (void)hipGraphDestroy(g);
        HIPCHK(hipGraphLaunch(gx, c->stream));  // warm-up replay
    }
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    HIPCHK(hipEventRecord(e0, c->stream));
    if (gx) HIPCHK(hipGraphLaunch(gx, c->stream));
    else for (int i = 0; i < reps; ++i) run();
    HIPCHK(hipEventRecord(e1, c->stream));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (gx) (void)hipGraphExecDestroy(gx);
    HIPCHK(hipGetLastError());
    *ms_per_launch = ms / reps;
    return fuse_err(c);
}

// L (op 0) or L^T (op 1) with the launches cycling over `nsets` input / output buffer pairs:
// with nsets (|P| + |D|) scalars beyond the 256 MiB Infinity Cache, every launch reads its
// input from HBM (the repeated-buffer op_bench is L3-assisted once a working set fits)
int raocp_op_bench_rot(raocp_ctx* c, int op, int reps, int nsets, float* ms_per_launch) {
    DevGuard dg_(c);
    SweepLock sl_(c);
    if (!c || reps < 1 || nsets < 1 || nsets > 16 || !ms_per_launch || (op != 0 && op != 1))
        return fail(RAOCP_ERR_ARG, "bad argument");
    if (int ra = ell_available(c)) return ra;
    if (int rci = bench_inputs(c)) return rci;
    std::vector<DevMem> mem(2 * (size_t)nsets);  // freed at every return
    std::vector<double*> P(nsets), D(nsets);
    for (int k = 0; k < nsets; ++k) {
        DevMem &a = mem[2 * k], &b = mem[2 * k + 1];
        if (a.alloc(c->P * c->wsz + 64) != hipSuccess || b.alloc(c->D * c->wsz + 64) != hipSuccess)
            return fail(RAOCP_ERR_HIP, "hipMalloc (rotating buffer sets)");
        P[k] = (double*)a.p;
        D[k] = (double*)b.p;
        (void)hipMemcpyAsync(P[k], c->tmpP, c->P * c->wsz, hipMemcpyDeviceToDevice, c->stream);
        (void)hipMemcpyAsync(D[k], c->tmpD, c->D * c->wsz, hipMemcpyDeviceToDevice, c->stream);
    }
    auto run = [&](int i) {
        const int k = i % nsets;
        if (op == 0) launch_ell(c, P[k], D[k]);
        else launch_ell_t(c, D[k], P[k]);
    };
    for (int i = 0; i < nsets; ++i) run(i);  // warm-up
    hipGraphExec_t gx = nullptr;
    hipGraph_t g = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    float ms = 0;
    bool ok = hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
    if (ok) {
        for (int i = 0; i < reps; ++i) run(i);
        ok = hipStreamEndCapture(c->stream, &g) == hipSuccess && hipGraphInstantiate(&gx, g, nullptr, nullptr, 0) == hipSuccess;
    }
    if (g) (void)hipGraphDestroy(g);
    ok = ok && hipGraphLaunch(gx, c->stream) == hipSuccess;  // warm-up replay
    ok = ok && hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess;
    ok = ok && hipEventRecord(e0, c->stream) == hipSuccess && hipGraphLaunch(gx, c->stream) == hipSuccess &&
         hipEventRecord(e1, c->stream) == hipSuccess && hipEventSynchronize(e1) == hipSuccess &&
         hipEventElapsedTime(&ms, e0, e1) == hipSuccess;
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (gx) (void)hipGraphExecDestroy(gx);
    (void)hipStreamSynchronize(c->stream);
    mem.clear();
    if (!ok) return fail(RAOCP_ERR_HIP, std::string("op_bench_rot: ") + hipGetErrorString(hipGetLastError()));
    *ms_per_launch = ms / reps;
    return RAOCP_OK;
}

}  // extern "C"
