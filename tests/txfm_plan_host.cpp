// Host build of svt-av1_amd/csrc/txfm_plan.h for tests/test_txfm_plan_host.py.
//     txfm_plan_host                      -> one line per transform size:  size <ts> <class> <teams>
//     txfm_plan_host <ts>:<nblk> ...      -> one line per launch of the plan for these jobs, in issue order:
//                                            launch <class> <njobs> jobs <index> ... wg <first_wg[0]> ... <first_wg[njobs]>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../svt-av1_amd/csrc/txfm_plan.h"

int main(int argc, char** argv) {
    if (argc == 1) {
        for (int ts = 0; ts < kTxSizes; ts++) printf("size %d %d %d\n", ts, tx_plan_class(ts), tx_plan_teams(ts));
        return 0;
    }
    std::vector<int> ts, nblk;
    for (int i = 1; i < argc; i++) {
        int a = 0, b = 0;
        if (sscanf(argv[i], "%d:%d", &a, &b) != 2) return 2;
        ts.push_back(a); nblk.push_back(b);
    }
    for (const TxPlanLaunch& l : tx_plan(ts.data(), nblk.data(), (int)ts.size())) {
        printf("launch %d %d jobs", l.cls, l.njobs);
        for (int j = 0; j < l.njobs; j++) printf(" %d", l.job[j]);
        printf(" wg");
        for (int j = 0; j <= l.njobs; j++) printf(" %d", l.first_wg[j]);
        printf("\n");
    }
    return 0;
}
