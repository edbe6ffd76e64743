// raocp_tile.h — the tile layer of the streaming kernels, defined once for every translation
// unit: raocp_capi.hip (through raocp_kernels.hip: k_cp3 and its weight image k_cp3_image, the
// node-block kernels of raocp_cp2.hip / raocp_cp.hip, raocp_ell2/3.hip, raocp_dyn2/3.hip),
// raocp_cp4.hip, raocp_cp5.hip and raocp_dynr.hip. Family / leaf tiles of 16 nodes, lane
// lo = node, lane group h = lane >> 4 holding rows KC h .. KC h + KC - 1 of an R-row vector,
// R = 4 KC ("row layout", raocp_cp3.hip); products in the transposed MFMA form D = W V with the
// weights as the A operand from the weight image in LDS. WL is that image's layout contract:
// k_cp3_image writes it through WL::fill, k_cp3 / k_cp4 / k_cp5 / k_cp6 / k_drc read it through
// WL::get. Header-only, anonymous namespace: each translation unit gets its own copies.
#pragma once

#include "raocp_common.h"

namespace raocp {
namespace {

template <class U>
using glbp = __attribute__((address_space(1))) U*;
template <class U>
using cglbp = const __attribute__((address_space(1))) U*;

// ---- 16x16x4 MFMA in T ----------------------------------------------------------------
template <class T>
struct MF;
template <>
struct MF<double> {
    typedef double v4 __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ v4 mma(double a, double b, v4 c) {
        return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
    }
    // tile row (A row) of accumulator element e in lane group h = lane >> 4, and back
    static __device__ __forceinline__ int row(int h, int e) { return h + 4 * e; }
    static __device__ __forceinline__ int h_of(int a) { return a & 3; }
    static __device__ __forceinline__ int e_of(int a) { return a >> 2; }
};
template <>
struct MF<float> {
    typedef float v4 __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ v4 mma(float a, float b, v4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ int row(int h, int e) { return 4 * h + e; }
    static __device__ __forceinline__ int h_of(int a) { return a >> 2; }
    static __device__ __forceinline__ int e_of(int a) { return a & 3; }
};

// A row lo of an output row tile lands in lane group g, register e of the accumulator
template <class T>
struct MFA;
template <>
struct MFA<double> {  // D row = h + 4 e
    static __device__ __forceinline__ int g_of(int lo) { return lo & 3; }
    static __device__ __forceinline__ int e_of(int lo) { return lo >> 2; }
};
template <>
struct MFA<float> {  // D row = 4 h + e
    static __device__ __forceinline__ int g_of(int lo) { return lo >> 2; }
    static __device__ __forceinline__ int e_of(int lo) { return lo & 3; }
};
// the weight row A row lo of output row tile ro carries for an R-row output (-1: padding)
template <class T, int R>
__device__ __forceinline__ int wrow(int ro, int lo) {
    constexpr int KC = R / 4;
    const int t = 4 * ro + MFA<T>::e_of(lo);
    return t < KC ? KC * MFA<T>::g_of(lo) + t : -1;
}

// weight fragments of one R x K table (column-major M[k R + r]) in the transposed form, staged
// once per workgroup in LDS: lds[(ro KS + s) 64 + lane] = M[wrow(ro, lo)][K/4 h + s]. fill()
// writes that order (k_cp3_image), get() reads it: the one definition of the image's layout.
template <class T, int R, int K>
struct WL {
    static_assert(R % 4 == 0 && K % 4 == 0, "row layout: R, K multiples of 4");
    static constexpr int RO = (R / 4 + 3) / 4, KS = K / 4, N = RO * KS * 64;
    const __attribute__((address_space(3))) T* base;
    __device__ __forceinline__ T get(int ro, int s) const { return base[(ro * KS + s) * 64 + (threadIdx.x & 63)]; }
    // every thread of the workgroup takes part (a __syncthreads follows)
    template <class DP>
    static __device__ __forceinline__ void fill(DP dst, const T* tab, int t) {
        cglbp<T> M = (cglbp<T>)(tab + (size_t)t * R * K);
        for (int q = threadIdx.x; q < N; q += blockDim.x) {
            const int l = q & 63, lo = l & 15, h = l >> 4, s = (q >> 6) % KS, ro = (q >> 6) / KS;
            const int r = wrow<T, R>(ro, lo), k = KS * h + s;
            dst[q] = r >= 0 ? M[k * R + r] : T(0);
        }
    }
    // the same table behind an opaque base: a product through it re-reads its fragments from
    // LDS instead of keeping an earlier product's (RO KS registers) live in between
    __device__ __forceinline__ WL fresh() const {
        const __attribute__((address_space(3))) T* b = base;
        asm volatile("" : "+v"(b));
        return WL{b};
    }
};
// acc[ro] += W b (b in row layout over K)
template <class T, int R, int K>
__device__ __forceinline__ void mmt(const WL<T, R, K>& W, const T (&b)[(K + 15) / 16][4],
                                    typename MF<T>::v4 (&acc)[(R + 15) / 16]) {
    _Pragma("unroll") for (int s = 0; s < WL<T, R, K>::KS; ++s)
        _Pragma("unroll") for (int ro = 0; ro < WL<T, R, K>::RO; ++ro)
            acc[ro] = MF<T>::mma(W.get(ro, s), b[s >> 2][s & 3], acc[ro]);
}

// 4 consecutive T at 4- / 8-B alignment (node rows start wherever the flat layout puts them)
template <class T>
struct V4a {
    typedef T type __attribute__((ext_vector_type(4), aligned(sizeof(T))));
};
// slot (rt, e) of an R-row vector holds a row (t = 4 rt + e < R / 4)
template <int R>
__device__ __forceinline__ constexpr bool tok(int rt, int e) {
    return 4 * rt + e < R / 4;
}
// row-layout load of an R-row node vector: a[rt][e] = v[R/4 h + 4 rt + e] (0 past R/4).
// v must be a valid row address even when !live: every load is issued unconditionally and
// the value selected after it -- a load under a runtime condition makes the compiler branch
// around it and wait for it on its own, one memory round trip per load
template <class T, int R>
__device__ __forceinline__ void ld_rows(cglbp<T> v, bool live, T (&a)[(R + 15) / 16][4]) {
    typedef typename V4a<T>::type vt;
    constexpr int KC = R / 4;
    cglbp<T> b = v + KC * ((threadIdx.x & 63) >> 4);
    _Pragma("unroll") for (int rt = 0; rt < (R + 15) / 16; ++rt) {
        if (4 * rt + 3 < KC) {
            const vt w = *(const __attribute__((address_space(1))) vt*)(b + 4 * rt);
            _Pragma("unroll") for (int e = 0; e < 4; ++e) a[rt][e] = live ? w[e] : T(0);
        } else {
            _Pragma("unroll") for (int e = 0; e < 4; ++e) {
                T w = T(0);
                if (tok<R>(rt, e)) w = b[4 * rt + e];
                a[rt][e] = live ? w : T(0);
            }
        }
    }
}
// ld_rows with the loads themselves under `live` (v need not be valid when !live): the form of
// k_cp3 and the raocp_dyn3.hip kernels; k_cp4 / k_cp5 / k_cp6 / k_dr / k_drc use ld_rows, whose
// unconditional loads the compiler does not branch around
template <class T, int R>
__device__ __forceinline__ void ld_rows_g(cglbp<T> v, bool live, T (&a)[(R + 15) / 16][4]) {
    typedef typename V4a<T>::type vt;
    constexpr int KC = R / 4;
    cglbp<T> b = v + KC * ((threadIdx.x & 63) >> 4);
    _Pragma("unroll") for (int rt = 0; rt < (R + 15) / 16; ++rt) {
        if (live && 4 * rt + 3 < KC) {
            const vt w = *(const __attribute__((address_space(1))) vt*)(b + 4 * rt);
            _Pragma("unroll") for (int e = 0; e < 4; ++e) a[rt][e] = w[e];
        } else {
            _Pragma("unroll") for (int e = 0; e < 4; ++e) a[rt][e] = (live && tok<R>(rt, e)) ? b[4 * rt + e] : T(0);
        }
    }
}
// one scalar at a valid address, zero when !live (unconditional load, see ld_rows)
template <class T>
__device__ __forceinline__ T ldz(cglbp<T> v, bool live) {
    const T w = *v;
    return live ? w : T(0);
}
template <class T, int R>
__device__ __forceinline__ void st_rows(glbp<T> v, bool live, const T (&a)[(R + 15) / 16][4]) {
    typedef typename V4a<T>::type vt;
    constexpr int KC = R / 4;
    glbp<T> b = v + KC * ((threadIdx.x & 63) >> 4);
    _Pragma("unroll") for (int rt = 0; rt < (R + 15) / 16; ++rt) {
        if (!live) continue;
        if (4 * rt + 3 < KC) {
            vt w;
            _Pragma("unroll") for (int e = 0; e < 4; ++e) w[e] = a[rt][e];
            *(__attribute__((address_space(1))) vt*)(b + 4 * rt) = w;
        } else {
            _Pragma("unroll") for (int e = 0; e < 4; ++e)
                if (tok<R>(rt, e)) b[4 * rt + e] = a[rt][e];
        }
    }
}
// the same from LDS rows (the box bounds of one-table trees)
template <class T, int R>
__device__ __forceinline__ void ld_rows_lds(const __attribute__((address_space(3))) T* v, T (&a)[(R + 15) / 16][4]) {
    constexpr int KC = R / 4;
    const __attribute__((address_space(3))) T* b = v + KC * ((threadIdx.x & 63) >> 4);
    _Pragma("unroll") for (int rt = 0; rt < (R + 15) / 16; ++rt)
        _Pragma("unroll") for (int e = 0; e < 4; ++e) a[rt][e] = tok<R>(rt, e) ? b[4 * rt + e] : T(0);
}

// 32-bit element offsets from a wave-uniform base: loads and stores through el() / elw()
// address with the SGPR base and a 32-bit VGPR byte offset (global_* saddr), so no 64-bit
// per-lane pointer has to stay live across a tile loop (byte offsets below 4 GiB)
template <class T>
__device__ __forceinline__ cglbp<T> el(cglbp<T> b, unsigned o) {
    return (cglbp<T>)((const __attribute__((address_space(1))) char*)b + o * (unsigned)sizeof(T));
}
template <class T>
__device__ __forceinline__ glbp<T> elw(glbp<T> b, unsigned o) {
    return (glbp<T>)((__attribute__((address_space(1))) char*)b + o * (unsigned)sizeof(T));
}
// ld_rows / st_rows / ldz at element offset off from base
template <class T, int R>
__device__ __forceinline__ void ld_rows_o(cglbp<T> base, unsigned off, bool live, T (&a)[(R + 15) / 16][4]) {
    typedef typename V4a<T>::type vt;
    constexpr int KC = R / 4;
    const unsigned o = off + KC * ((threadIdx.x & 63) >> 4);
    _Pragma("unroll") for (int rt = 0; rt < (R + 15) / 16; ++rt) {
        if (4 * rt + 3 < KC) {
            const vt w = *(const __attribute__((address_space(1))) vt*)el(base, o + 4 * rt);
            _Pragma("unroll") for (int e = 0; e < 4; ++e) a[rt][e] = live ? w[e] : T(0);
        } else {
            _Pragma("unroll") for (int e = 0; e < 4; ++e) {
                T w = T(0);
                if (tok<R>(rt, e)) w = *el(base, o + 4 * rt + e);
                a[rt][e] = live ? w : T(0);
            }
        }
    }
}
template <class T, int R>
__device__ __forceinline__ void st_rows_o(glbp<T> base, unsigned off, bool live, const T (&a)[(R + 15) / 16][4]) {
    typedef typename V4a<T>::type vt;
    constexpr int KC = R / 4;
    const unsigned o = off + KC * ((threadIdx.x & 63) >> 4);
    _Pragma("unroll") for (int rt = 0; rt < (R + 15) / 16; ++rt) {
        if (!live) continue;
        if (4 * rt + 3 < KC) {
            vt w;
            _Pragma("unroll") for (int e = 0; e < 4; ++e) w[e] = a[rt][e];
            *(__attribute__((address_space(1))) vt*)elw(base, o + 4 * rt) = w;
        } else {
            _Pragma("unroll") for (int e = 0; e < 4; ++e)
                if (tok<R>(rt, e)) *elw(base, o + 4 * rt + e) = a[rt][e];
        }
    }
}
template <class T>
__device__ __forceinline__ T ldz_o(cglbp<T> base, unsigned off, bool live) {
    const T w = *el(base, off);
    return live ? w : T(0);
}

// sum over the 4 lane groups (the rows of one node). RAOCP_SUMH_SHFL (defined by a translation
// unit before this header) selects the shuffle form: raocp_dynr.hip (the row swaps spill in
// k_drc) and raocp_capi.hip (k_cp3 as it was written)
template <class T>
__device__ __forceinline__ T sum_h(T v) {
#ifdef RAOCP_SUMH_SHFL
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
#endif
    // lanes l ^ 16 and l ^ 32 by gfx950's row swaps (v_permlane16_swap / v_permlane32_swap: VALU
    // moves, no LDS round trip as ds_bpermute); every lane adds its own value and its partner's,
    // so the four lane groups end with the same sum, as with the shuffles
    if constexpr (sizeof(T) == 8) {
        auto sw16 = [](T x) {
            const auto lo = __builtin_amdgcn_permlane16_swap(__double2loint(x), __double2loint(x), false, false);
            const auto hi = __builtin_amdgcn_permlane16_swap(__double2hiint(x), __double2hiint(x), false, false);
            return __hiloint2double(hi[0], lo[0]) + __hiloint2double(hi[1], lo[1]);
        };
        auto sw32 = [](T x) {
            const auto lo = __builtin_amdgcn_permlane32_swap(__double2loint(x), __double2loint(x), false, false);
            const auto hi = __builtin_amdgcn_permlane32_swap(__double2hiint(x), __double2hiint(x), false, false);
            return __hiloint2double(hi[0], lo[0]) + __hiloint2double(hi[1], lo[1]);
        };
        return sw32(sw16(v));
    } else {
        const auto a = __builtin_amdgcn_permlane16_swap(__float_as_int(v), __float_as_int(v), false, false);
        const T w = __int_as_float(a[0]) + __int_as_float(a[1]);
        const auto b = __builtin_amdgcn_permlane32_swap(__float_as_int(w), __float_as_int(w), false, false);
        return __int_as_float(b[0]) + __int_as_float(b[1]);
    }
}

// per-wave scratch of the kernel projection: the family's y (2C + 1 <= 9) and the children's
// tau, s after the L^T half step (phase 5 reads them across lane groups)
template <class T>
struct KpScratch {
    T y[16][9];
    T tau[16][4];
    T s[16][4];
};

__device__ __forceinline__ void dma_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// the weight image (or a part of it) by LDS-DMA: `chunks` 16-B pieces from src to dst, every
// wave of the workgroup issuing its share (the caller waits with dma_wait + a barrier)
__device__ __forceinline__ void lds_fill(ldsd* dst, const double* src, int chunks) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int c0 = wv * 64; c0 < chunks; c0 += nw * 64) {
        const int ch = c0 + lane;
        if (ch < chunks)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) double*)(src + 2 * ch), dst + 2 * c0,
                                             16, 0, 0);
    }
}

}  // namespace
}  // namespace raocp
