// ifa_gemm_plan_capi.hip -- the prompt GEMM launch plans (ifa_gemm_plan.h) and the MoE layer plan (ifa_moe_plan.h) behind the C ABI, for
// tests: the pure functions, no device is touched.
#include <cstring>
#include "ifa_host.h"
#include "ifa_gemm_plan.h"
#include "ifa_gemm_rows_plan.h"
#include "ifa_moe_plan.h"

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

} // extern "C"
