// i8joint_check — the joint-row arithmetic of the int8 tail copy (csrc/knn_plan.h
// i8t_joint_row_bytes, i8t_tail_stages, i8t_row_stages) printed over a grid of (head, dpt) pairs,
// valid and invalid, one line each: "head dpt row_bytes tail_stages row_stages".
// tests/test_i8joint_cpu.py compiles it with knn_plan.cpp (HIP-free) under sanitizers and compares
// every line with its own statement of the layout.
#include <cstdio>

#include "../../image_recommender_amd/csrc/knn_plan.h"

int main() {
    using namespace imgrec;
    for (int head = -64; head <= 2112; head += 32)
        for (int dpt = 0; dpt <= 4224; dpt += 64)
            std::printf("%d %d %d %d %d\n", head, dpt, i8t_joint_row_bytes(head, dpt), i8t_tail_stages(dpt),
                        i8t_row_stages(head, dpt));
    return 0;
}
