// ifa_pool_rows_plan.h -- which pooled rows a step serves, and in which launches (pure: no HIP, no device; the C ABI exposes it for
// tests as ifa_pool_rows_plan).  A pool call names its rows once, ascending (rows_sel [n_sel], indices into the call's n rows); the
// call may run as several steps (chunks of a batched step), each over the call's rows [chunk0, chunk0 + n_rows).  A step serves the
// pooled rows that fall into its rows, from the call's cursor on, and cuts them into maximal runs of equal "armed" (adj[j] >= 0: the
// row passes through the logit processors of state slot adj[j] first): one run = one "[adjust ->] pool [-> lse]" group of launches.
// A run never crosses a step: the rows of the next chunk are in another logits block.
#pragma once
#include <vector>

namespace ifa {

struct PoolRun { int ja, jb, armed; };      // pooled rows [ja, jb) of the call, all armed or all raw

// rows_sel [n_sel] ascending; adj [n_sel] or null (nothing armed); cursor: pooled rows served by the steps before this one.
// Returns the cursor behind this step; runs (cleared first) takes the step's runs in order.
static inline int pool_rows_plan(const int *rows_sel, const int *adj, int n_sel, int cursor, int chunk0, int n_rows, std::vector<PoolRun> &runs)
{
    runs.clear();
    int j1 = cursor;
    while (j1 < n_sel && rows_sel[j1] < chunk0 + n_rows) j1++;
    for (int ja = cursor; ja < j1;) {
        const int armed = (adj && adj[ja] >= 0) ? 1 : 0;
        int jb = ja + 1;
        while (jb < j1 && ((adj && adj[jb] >= 0) ? 1 : 0) == armed) jb++;
        runs.push_back(PoolRun{ja, jb, armed});
        ja = jb;
    }
    return j1;
}

} // namespace ifa
