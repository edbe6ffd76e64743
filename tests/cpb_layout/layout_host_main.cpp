// Stand-alone host program: the slab map of the batched CP kernel (csrc/raocp_cpb_layout.h, no
// HIP dependency) for both element sizes.
//
//   layout_host P D n m nx nu [P D n m nx nu ...]
//
// For every problem and for elements of 8 and 4 bytes it checks that every array starts on a
// 16-byte boundary, that the arrays are in order and do not overlap (each holds its length), that
// the last one ends within the stride, and that the stride is a multiple of 256 bytes; and that
// the float slab is no larger in bytes than the double one. Prints one line per map and
// "<failures> of <checks> layout checks failed"; the exit code is the number of failures (capped).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "raocp_cpb_layout.h"

namespace {

int g_checks = 0, g_fail = 0;

void check(bool ok, const char* what, long a, long b) {
    ++g_checks;
    if (!ok) {
        ++g_fail;
        std::printf("  FAILED: %s (%ld, %ld)\n", what, a, b);
    }
}

struct Arr {
    const char* name;
    long off, len;
};

long check_map(long P, long D, long n, long m, long nx, long nu, int elt) {
    const raocp::CpbSlab L = raocp::cpb_layout_dims(P, D, n, m, nx, nu, elt);
    const std::vector<Arr> arrs = {{"z0", L.z[0], P},      {"z1", L.z[1], P},          {"z2", L.z[2], P},
                                   {"e0", L.e[0], D},      {"e1", L.e[1], D},          {"xi2", L.xi2, D},
                                   {"tv", L.tv, D},        {"q", L.q, n * nx},         {"dd", L.dd, m * nu},
                                   {"pb", L.pb, n * (nx + nu)}, {"x0", L.x0, nx}};
    check(arrs[0].off == 0, "the first primal starts the slab", arrs[0].off, 0);
    for (size_t i = 0; i < arrs.size(); ++i) {
        check(arrs[i].off >= 0 && (arrs[i].off * elt) % 16 == 0, arrs[i].name, arrs[i].off, elt);
        const long next = i + 1 < arrs.size() ? arrs[i + 1].off : L.stride;
        check(arrs[i].off + arrs[i].len <= next, "array overlaps the next one", arrs[i].off + arrs[i].len, next);
        // what the 16-byte loops of k_mpc_step move past an array's end stays before the next array
        check(((arrs[i].off + arrs[i].len) * elt + 15) / 16 * 16 <= next * elt, "16-byte tail crosses into the next array",
              arrs[i].off + arrs[i].len, next);
    }
    check(L.stride > 0 && (L.stride * elt) % 256 == 0, "stride is not a multiple of 256 bytes", L.stride, elt);
    std::printf("P %ld D %ld n %ld m %ld nx %ld nu %ld elt %d: stride %ld elements, %ld bytes\n", P, D, n, m, nx, nu, elt,
                L.stride, L.stride * elt);
    return L.stride * elt;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 7 || (argc - 1) % 6 != 0) {
        std::printf("usage: %s P D n m nx nu [...]\n", argv[0]);
        return 99;
    }
    for (int i = 1; i + 5 < argc; i += 6) {
        long v[6];
        for (int k = 0; k < 6; ++k) v[k] = std::atol(argv[i + k]);
        const long b8 = check_map(v[0], v[1], v[2], v[3], v[4], v[5], 8);
        const long b4 = check_map(v[0], v[1], v[2], v[3], v[4], v[5], 4);
        check(b4 <= b8, "the float slab is larger than the double slab", b4, b8);
    }
    std::printf("%d of %d layout checks failed\n", g_fail, g_checks);
    return g_fail > 98 ? 98 : g_fail;
}
