// raocp_cpb_layout.h — the memory map of one instance's slab of the batched CP kernel
// (raocp_cpb.hip) as pure host arithmetic: no HIP dependency, so a host-only program can
// include it (tests/cpb_layout/layout_host_main.cpp).
#pragma once

namespace raocp {

// one instance's slab in HBM: offsets in ELEMENTS of the context's scalar type (double, or
// float on an fp32 context) from the slab's start, every array on a 16-B boundary, `stride`
// elements (a multiple of 256 B) between the slabs of two instances
struct CpbSlab {
    long z[3];    // the rotating primals (P each)
    long e[2];    // the rotating duals (D each)
    long xi2;     // xi2 (D)
    long tv;      // the dual half step v before its projection (D)
    long q;       // q rows of the dynamics projection (n x nx)
    long dd;      // d rows (m x nu)
    long pb;      // child products [h | a] (n x (nu + nx))
    long x0;      // the instance's initial state (nx)
    long stride;
};

// the map for a tree of n nodes (m nonleaf), primal length P, dual length D and elements of
// `elt` bytes (8 or 4): every array length is rounded up to 16 B (2 doubles, 4 floats) and the
// stride to 256 B (32 doubles, 64 floats); the 16-B copy and clear loops of k_mpc_step rely on both
inline CpbSlab cpb_layout_dims(long P, long D, long n, long m, long nx, long nu, int elt) {
    CpbSlab L{};
    const long unit = 16 / elt, line = 256 / elt;
    long at = 0;
    auto take = [&](long count) {
        const long o = at;
        at += (count + unit - 1) / unit * unit;
        return o;
    };
    for (int b = 0; b < 3; ++b) L.z[b] = take(P);
    for (int b = 0; b < 2; ++b) L.e[b] = take(D);
    L.xi2 = take(D);
    L.tv = take(D);
    L.q = take(n * nx);
    L.dd = take(m * nu);
    L.pb = take(n * (nx + nu));
    L.x0 = take(nx);
    L.stride = (at + line - 1) / line * line;
    return L;
}

}  // namespace raocp
