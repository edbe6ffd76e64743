// raocp_cpa_layout.h — the memory map of one instance's second slab, the state of the
// Anderson acceleration of k_cpa (raocp_cpb.hip), as pure host arithmetic: no HIP dependency,
// so a host-only program can include it (tests/accel/aa_host_main.cpp). The CP iterate itself
// stays in the instance's CpbSlab (raocp_cpb_layout.h).
#pragma once

namespace raocp {

// the small state block at CpaSlab::state (4 doubles of room)
struct CpaState {
    int head;      // the ring slot the next column goes to
    int count;     // columns held (<= m)
    int have;      // 1: pg / pr hold the pair the next column is a difference from
    int pending;   // 1: the iterate is a proposal; sg holds g_k and rnorm |r_k|_2
    double rnorm;
};

// one instance's slab in HBM: offsets in doubles from the slab's start, every array on a 16-B
// boundary, `stride` doubles (a multiple of 256 B) between the slabs of two instances. A vector
// is the primal (P) followed by the dual (D).
struct CpaSlab {
    long dg;       // m columns dG_i = g_{i+1} - g_i, `vec` doubles apart, in ring slots
    long dr;       // m columns dR_i = r_{i+1} - r_i
    long pg;       // the previous g
    long pr;       // the previous r
    long sg;       // g_k as it was when a proposal replaced it
    long G;        // dR' dR by ring slot, 8 x 8
    long state;    // CpaState
    long vec;      // doubles of one vector: P + D rounded up to 16 B
    long stride;
    int m;
};

inline CpaSlab cpa_layout_dims(long P, long D, int m) {
    CpaSlab L{};
    const long unit = 2, line = 32;
    L.m = m;
    L.vec = (P + D + unit - 1) / unit * unit;
    long at = 0;
    auto take = [&](long count) {
        const long o = at;
        at += (count + unit - 1) / unit * unit;
        return o;
    };
    L.dg = take(m * L.vec);
    L.dr = take(m * L.vec);
    L.pg = take(L.vec);
    L.pr = take(L.vec);
    L.sg = take(L.vec);
    L.G = take(64);
    L.state = take((long)((sizeof(CpaState) + 7) / 8));
    L.stride = (at + line - 1) / line * line;
    return L;
}

}  // namespace raocp
