// energy_carry_plan_check.cpp -- the carry plan of the register-resident energy kernel (dsp_internal_plan_energy_carries, dsp_plan.cpp)
// for a few thousand random parameter sets and every edge value, against a restatement by brute force, built with
// -fsanitize=address,undefined (tests/test_energy_carry_plan_cpu.py compiles and runs it).
//
//     energy_carry_plan_check <sets> <seed>        prints one JSON line; exit status 1 on the first difference
//
// The restatement walks the samples instead of dividing: sub-chain s of lane j starts at sample j C + s CS of the row, its lagged window
// `lag` samples lower; stepping down lane by lane finds the lane whose chunk holds that sample and how many samples r of the chunk lie
// in front of it; counting r samples off in groups of 8 finds the group of sample r - 1, the number of whole groups in front of it and
// the samples pn of the group.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "../dspeed_amd/csrc/dsp_plan.h"

static long checked = 0;

static bool check(int C, int S, const int32_t lags[3]) {
    EnergyPlan* plan = new EnergyPlan;  // (on the heap: a write past the struct is the sanitizer's to see)
    memset(plan, 0x5a, sizeof *plan);
    dsp_internal_plan_energy_carries(C, S, lags, plan);
    const int CS = (C - 2) / S;
    bool ok = true;
    for (int k = 0; k < 3 && ok; ++k)
        for (int s = 0; s < S && ok; ++s) {
            long pos = (long)s * CS - lags[k];  // relative to the start of the lane's chunk
            int shift = 0;
            while (pos < 0) {
                pos += C;
                ++shift;
            }
            const int r = (int)pos;
            int group = 0, in_front = 0, pn = 0;
            for (int i = 0; i < r; ++i) {  // sample i of the chunk lies in front of the capture point
                if (pn == 8) {
                    ++group;
                    in_front = group;
                    pn = 0;
                }
                ++pn;
            }
            const int side = in_front - 1;
            ++checked;
            if (plan->cs[k][s] * CS + plan->local[k][s] != r) {
                printf("C=%d S=%d lag=%d s=%d: cs %d local %d are not r = %d\n", C, S, lags[k], s, plan->cs[k][s], plan->local[k][s], r);
                ok = false;
            }
            if (plan->shift[k][s] != shift || plan->grp[k][s] != 8 * group || plan->side[k][s] != side || plan->pn[k][s] != pn) {
                printf("C=%d S=%d lag=%d s=%d: plan shift %d grp %d side %d pn %d, brute force %d %d %d %d\n", C, S, lags[k], s, plan->shift[k][s],
                       plan->grp[k][s], plan->side[k][s], plan->pn[k][s], shift, 8 * group, side, pn);
                ok = false;
            }
            // what the kernel relies on: the four pairs it reads start inside the chunk, the side array element exists, 0 <= pn <= 8
            if (plan->grp[k][s] < 0 || plan->grp[k][s] > C - 2 || plan->side[k][s] < -1 || plan->side[k][s] > (C - 2) / 8 - 1 || plan->pn[k][s] < 0 ||
                plan->pn[k][s] > 8 || plan->shift[k][s] < 0) {
                printf("C=%d S=%d lag=%d s=%d: out of the kernel's range\n", C, S, lags[k], s);
                ok = false;
            }
        }
    delete plan;
    return ok;
}

int main(int argc, char** argv) {
    const long sets = argc > 1 ? atol(argv[1]) : 4000;
    std::mt19937 rng(argc > 2 ? (unsigned)atol(argv[2]) : 1u);
    const int lens[4] = {1024, 2048, 4096, 8192};
    for (int li = 0; li < 4; ++li) {  // every lag that puts the capture point on an edge value, at shift 0 .. 3
        const int C = lens[li] / 64 + 2;
        const int edges[6] = {0, 1, 8, 9, C - 2, C - 1};
        for (int S = 1; S <= 2; ++S)
            for (int e = 0; e < 6; ++e)
                for (int sh = 0; sh < 4; ++sh) {
                    const int lag = sh * C + (C - edges[e]) % C;
                    const int32_t lags[3] = {lag > 0 ? lag : C, lag + 1, 2 * lag + 1};
                    if (!check(C, S, lags)) return 1;
                }
    }
    for (long i = 0; i < sets; ++i) {
        const int len = lens[rng() % 4], C = len / 64 + 2, S = 1 + (int)(rng() % 2);
        const int rise = 1 + (int)(rng() % (len / 2)), flat = (int)(rng() % (len - 2 * rise + 1)), fall = 1 + (int)(rng() % (len - rise - flat));
        const int32_t lags[3] = {rise, rise + flat, (rng() & 1) ? 2 * rise + flat : rise + flat + fall};
        if (!check(C, S, lags)) return 1;
    }
    printf("{\"sets\": %ld, \"entries\": %ld}\n", sets, checked);
    return 0;
}
