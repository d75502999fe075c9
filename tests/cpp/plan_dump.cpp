// plan_dump -- prints the projection planner's answers (csrc/wide_plan.cpp) for tests/test_wproj_plan.py.
// Host code only: built with the C++ compiler from wide_plan.cpp alone, no library and no GPU.
//
// stdin:  one query per line, `rows K LP v2 nn fp8`
// stdout: one line per query, `blocks splits chunk merge s8_scaled <kernel of the hi / lo product>
//         <kernel of the single-panel product>`
#include <cstdio>

#include "wide.hpp"

int main() {
    long long rows, K;
    int LP, v2, nn, fp8;
    while (std::scanf("%lld %lld %d %d %d %d", &rows, &K, &LP, &v2, &nn, &fp8) == 6) {
        const rsvd::WProjPlan p = rsvd::plan_wproj(rows, K, LP, v2 != 0, nn != 0, fp8 != 0);
        if (!rsvd::wproj_plan_valid(p)) {
            std::fprintf(stderr, "plan_wproj made a plan launch_wproj refuses: %lld %lld %d %d %d %d\n", rows, K, LP, v2, nn,
                         fp8);
            return 1;
        }
        std::printf("%d %d %lld %d %d %s %s\n", p.blocks, p.splits, (long long)p.chunk, (int)p.merge, (int)p.s8_scaled,
                    rsvd::wproj_kernel_name(rsvd::wproj_kernel_for(p, true)),
                    rsvd::wproj_kernel_name(rsvd::wproj_kernel_for(p, false)));
    }
    return 0;
}
