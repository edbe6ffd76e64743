// aa_count_main.cpp — host-only program over csrc/raocp_aa_ops.h: the classification of the
// acceleration's log records into the four counters k_mpc_step_aa keeps per MPC step (proposals
// made, trials accepted, trials rejected, solves refused). Built by tests/test_mpc_accel_host.py
// with -fsanitize=address,undefined.
//   aa_count LOG   LOG is a text file of records, kAaRec doubles each (code, j, prop, |r|_2,
//                  gamma[8]), as raocp_cp_batch_aa_log returns them
// The records are reduced as the kernel reduces them: 256 lanes stride over the rows, each lane
// keeps its own four counters, the lanes are added in index order. Prints "counts a b c d" and the
// number of records; exit code 1 when the file does not hold whole records.
#include <cstdio>
#include <vector>

#include "raocp_aa_ops.h"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    std::vector<double> log;
    double v;
    while (std::fscanf(f, "%lf", &v) == 1) log.push_back(v);
    std::fclose(f);
    if (log.size() % raocp::kAaRec != 0) {
        std::printf("%zu doubles are no whole number of records\n", log.size());
        return 1;
    }
    const int rows = (int)(log.size() / raocp::kAaRec), lanes = 256;
    std::vector<int> lane((size_t)lanes * raocp::kAaCounts, 0);
    for (int tid = 0; tid < lanes; ++tid)
        for (int r = tid; r < rows; r += lanes)
            raocp::aa_count((int)log[(size_t)r * raocp::kAaRec], (int)log[(size_t)r * raocp::kAaRec + 2],
                            &lane[(size_t)tid * raocp::kAaCounts]);
    int total[raocp::kAaCounts] = {0, 0, 0, 0};
    for (int tid = 0; tid < lanes; ++tid)
        for (int q = 0; q < raocp::kAaCounts; ++q) total[q] += lane[(size_t)tid * raocp::kAaCounts + q];
    std::printf("counts %d %d %d %d\nrecords %d\n", total[0], total[1], total[2], total[3], rows);
    return 0;
}
