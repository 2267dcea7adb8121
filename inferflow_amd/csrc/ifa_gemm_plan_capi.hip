// ifa_gemm_plan_capi.hip -- the prompt GEMM launch plans (ifa_gemm_plan.h), the MoE layer plan (ifa_moe_plan.h) and the pooled rows of
// a step (ifa_pool_rows_plan.h) behind the C ABI, for tests: the pure functions, no device is touched.
#include <cstring>
#include "ifa_host.h"
#include "ifa_gemm_plan.h"
#include "ifa_gemm_rows_plan.h"
#include "ifa_moe_plan.h"
#include "ifa_pool_rows_plan.h"

using namespace ifa;

extern "C" {

int ifa_gemm_mid_plan(const int *facts, int n_facts, int *out, int n_out)
{
    IFA_REQUIRE(facts && out && n_facts == GEMM_MID_N_FACTS && n_out >= GEMM_MID_N_OUT, "ifa_gemm_mid_plan: %d facts, %d outputs expected", GEMM_MID_N_FACTS, GEMM_MID_N_OUT);
    GemmMidFacts f;
    memcpy(&f, facts, sizeof(f));
    IFA_REQUIRE(f.num_cus >= 1, "ifa_gemm_mid_plan: num_cus %d", f.num_cus);
    const GemmMidPlan r = plan_gemm_mid(f);
    memcpy(out, &r, sizeof(r));
    return IFA_OK;
}

int ifa_gemm_big_plan(const int *facts, int n_facts, int *out, int n_out)
{
    IFA_REQUIRE(facts && out && n_facts == GEMM_BIG_N_FACTS && n_out >= GEMM_BIG_N_OUT, "ifa_gemm_big_plan: %d facts, %d outputs expected", GEMM_BIG_N_FACTS, GEMM_BIG_N_OUT);
    GemmBigFacts f;
    memcpy(&f, facts, sizeof(f));
    IFA_REQUIRE(f.num_cus >= 1, "ifa_gemm_big_plan: num_cus %d", f.num_cus);
    const GemmBigPlan r = plan_gemm_big(f);
    memcpy(out, &r, sizeof(r));
    return IFA_OK;
}

int ifa_gemm_rows_plan(const int *facts, int n_facts, int *out, int n_out)
{
    IFA_REQUIRE(facts && out && n_facts == GEMM_ROWS_N_FACTS && n_out >= GEMM_ROWS_N_OUT, "ifa_gemm_rows_plan: %d facts, %d outputs expected", GEMM_ROWS_N_FACTS, GEMM_ROWS_N_OUT);
    GemmRowsFacts f;
    memcpy(&f, facts, sizeof(f));
    IFA_REQUIRE(f.num_cus >= 1 && f.visible_cus >= 0, "ifa_gemm_rows_plan: num_cus %d, visible_cus %d", f.num_cus, f.visible_cus);
    const GemmRowsPlan r = plan_gemm_rows(f);
    memcpy(out, &r, sizeof(r));
    return IFA_OK;
}

// the plan of a mixture-of-experts layer (ifa_moe_plan.h): which grouped launches its products take
int ifa_moe_plan(const int *facts, int n_facts, int *out, int n_out)
{
    IFA_REQUIRE(facts && out && n_facts == MOE_N_FACTS && n_out >= MOE_N_OUT, "ifa_moe_plan: %d facts, %d outputs expected", MOE_N_FACTS, MOE_N_OUT);
    MoeFacts f;
    memcpy(&f, facts, sizeof(f));
    IFA_REQUIRE(f.T >= 1 && f.experts >= 1 && f.top_k >= 1, "ifa_moe_plan: %d rows, %d experts, top %d", f.T, f.experts, f.top_k);
    const MoePlan r = plan_moe_layer(f);
    memcpy(out, &r, sizeof(r));
    return IFA_OK;
}

// the pooled rows one step of a pool call serves, as runs of armed / raw rows (ifa_pool_rows_plan.h)
int ifa_pool_rows_plan(const int *rows_sel, const int *adj, int n_sel, int cursor, int chunk0, int n_rows, int *runs_out, int cap_runs, int *n_runs,
                       int *cursor_out)
{
    IFA_REQUIRE(n_sel >= 0 && (n_sel == 0 || rows_sel) && cursor >= 0 && cursor <= n_sel && chunk0 >= 0 && n_rows >= 0 && cap_runs >= 0
                && (cap_runs == 0 || runs_out) && n_runs && cursor_out, "ifa_pool_rows_plan: bad arguments");
    for (int j = 1; j < n_sel; j++) IFA_REQUIRE(rows_sel[j] > rows_sel[j - 1], "ifa_pool_rows_plan: rows_sel must be strictly ascending");
    std::vector<PoolRun> runs;
    *cursor_out = pool_rows_plan(rows_sel, adj, n_sel, cursor, chunk0, n_rows, runs);
    *n_runs = (int)runs.size();
    IFA_REQUIRE((int)runs.size() <= cap_runs, "ifa_pool_rows_plan: %zu runs, room for %d", runs.size(), cap_runs);
    for (size_t i = 0; i < runs.size(); i++) { runs_out[3 * i] = runs[i].ja; runs_out[3 * i + 1] = runs[i].jb; runs_out[3 * i + 2] = runs[i].armed; }
    return IFA_OK;
}

} // extern "C"
