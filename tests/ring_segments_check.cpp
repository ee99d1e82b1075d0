// The segment rule of the read-out ring's writer thread (shaderflow_amd/csrc/ring_segments.hpp), alone: a program of its own, built with
// the address and undefined-behaviour sanitizers by tests/test_host_opendml.py. Every line of the input is one case —
//     start budget gap count run[0] … run[count-1]
// — and the answer is a line with the frames in front of which a gap goes, then the position behind the last frame.
#include "ring_segments.hpp"

#include <cinttypes>
#include <cstdio>
#include <vector>

int main() {
    uint64_t start, budget, gap, count;
    while (scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &start, &budget, &gap, &count) == 4) {
        std::vector<uint64_t> runs(count);
        for (uint64_t& run : runs) if (scanf("%" SCNu64, &run) != 1) return 2;
        RingSegments rule;
        rule.begin(start, budget, gap);
        printf("cuts");
        for (uint64_t j = 0; j < count; j++) if (rule.cut(runs[j])) printf(" %" PRIu64, j);
        printf(" end %" PRIu64 "\n", rule.pos);
    }
    return 0;
}
