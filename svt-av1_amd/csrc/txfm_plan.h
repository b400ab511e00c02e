// txfm_plan.h — how a mixed-size transform call (svt_hip_launch_*_multi, txfm2d.hip) is cut into kernel launches.  Plain C++17, no HIP: the same text is
// built for the host by tests/test_txfm_plan_host.py.
//
// A mixed-size kernel instance holds the bodies of ONE class of transform sizes (classes by max(W, H)), so that its registers and its LDS tile are the class's own
// and not those of the 64-point body.  The plan sorts the caller's jobs into classes: jobs without blocks (or with a size outside 0..18) are dropped, the
// caller's order is kept within a class, a launch holds at most kTxPlanJobs jobs, and the launches come out class by class, the lightest class first.
#pragma once
#include <vector>

constexpr int kTxPlanJobs = 16;   // job lists per launch (the kernel argument holds this many)
constexpr int kTxSizes = 19;
constexpr int kTxPlanW[kTxSizes] = {4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64};
constexpr int kTxPlanH[kTxSizes] = {4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16};

// ---- the partition: class c holds the sizes with kTxClassTop[c - 1] < max(W, H) <= kTxClassTop[c].  <= 16 | >= 32, the light class launched first, is the
// grouping that measured best on the four-frame step (docs/kernels/transforms.md has the finer partitions' and the other order's numbers).
constexpr int kTxClasses = 2;
constexpr int kTxClassTop[kTxClasses] = {16, 64};

constexpr int tx_plan_long_side(int ts) { return kTxPlanW[ts] > kTxPlanH[ts] ? kTxPlanW[ts] : kTxPlanH[ts]; }
constexpr int tx_plan_class(int ts) {
    int c = 0;
    while (c + 1 < kTxClasses && tx_plan_long_side(ts) > kTxClassTop[c]) c++;
    return c;
}
// blocks per workgroup: 256 / max(W, H) lanes form a block team; 64x64 keeps two teams (its padded tile would not fit otherwise)
constexpr int tx_plan_teams(int ts) { return ts == 4 ? 2 : 256 / tx_plan_long_side(ts); }

struct TxPlanLaunch {
    int cls;                          // the kernel instance
    int njobs;                        // 1 .. kTxPlanJobs
    int job[kTxPlanJobs];             // indices into the caller's job array
    int first_wg[kTxPlanJobs + 1];    // prefix sums of ceil(nblk / teams); first_wg[njobs] = the grid size (> 0)
};

inline std::vector<TxPlanLaunch> tx_plan(const int* tx_size, const int* nblk, int njobs) {
    std::vector<TxPlanLaunch> plan;
    for (int cls = 0; cls < kTxClasses; cls++) {
        TxPlanLaunch l = {cls, 0, {}, {}};
        for (int j = 0; j <= njobs; j++) {
            const bool mine = j < njobs && nblk[j] > 0 && tx_size[j] >= 0 && tx_size[j] < kTxSizes && tx_plan_class(tx_size[j]) == cls;
            if (l.njobs && (j == njobs || (mine && l.njobs == kTxPlanJobs))) {   // the class is through, or the launch is full and another job waits
                plan.push_back(l);
                l = {cls, 0, {}, {}};
            }
            if (!mine) continue;
            const int t = tx_plan_teams(tx_size[j]);
            l.job[l.njobs++] = j;
            l.first_wg[l.njobs] = l.first_wg[l.njobs - 1] + (nblk[j] + t - 1) / t;
        }
    }
    return plan;
}
