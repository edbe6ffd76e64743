// Host driver of csrc/raocp_eval_ops.h (no HIP dependency): reads cases from stdin, one per line,
//   A <c> <alpha> <Z_0 .. Z_{c-1}> <p_0 .. p_{c-1}>   -> "A <value>" (avar_ru, %.17g)
//   F <c> <alpha> <Z ..> <p ..>                       -> the same with the probabilities held as float
//   P <count> <stage_ptr_0 .. stage_ptr_{count-1}>    -> "P <launches>" then one line per launch
//                                                        "L <s_hi> <s_lo> <blocks> <last>"
// Built by tests/test_eval_host.py with the host compiler and -fsanitize=address,undefined.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "raocp_eval_ops.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string kind;
        if (!(in >> kind)) continue;
        if (kind == "A" || kind == "F") {
            int c = 0;
            double alpha = 0.0;
            in >> c >> alpha;
            if (c < 1) return 2;
            std::vector<double> Z(c), p(c);
            for (double& v : Z) in >> v;
            for (double& v : p) in >> v;
            if (!in) return 2;
            double v;
            if (kind == "F") {
                const std::vector<float> pf(p.begin(), p.end());
                v = raocp::avar_ru(Z.data(), pf.data(), c, alpha);
            } else {
                v = raocp::avar_ru(Z.data(), p.data(), c, alpha);
            }
            printf("A %.17g\n", v);
        } else if (kind == "P") {
            int cnt = 0;
            in >> cnt;
            if (cnt < 2) return 2;
            std::vector<int> sp(cnt);
            for (int& v : sp) in >> v;
            if (!in) return 2;
            const std::vector<raocp::EvalLaunch> plan = raocp::eval_sweep_plan(sp);
            printf("P %zu\n", plan.size());
            for (const raocp::EvalLaunch& L : plan) printf("L %d %d %d %d\n", L.s_hi, L.s_lo, L.blocks, L.last ? 1 : 0);
        } else {
            return 2;
        }
    }
    return 0;
}
