// The MoE layer plan (csrc/ifa_moe_plan.h) as a stand-alone host program: the header alone, a plain C++17 compiler, no HIP.  A few plans
// with values written by hand, then the invariants over rows 1..512 x experts {4, 8, 64} x top_k {1, 2, 8} x every setting of the six
// options, the three tables and the four launcher predicates.  Exit code 0: all held.  (tests/test_moe_plan_cpu.py builds and runs it; it
// is also the program to build with -fsanitize=address,undefined.)
#include <cstdio>
#include "ifa_moe_plan.h"

using namespace ifa;

static int failures = 0;
#define EXPECT(cond)                                                                    \
    do {                                                                                \
        if (!(cond)) { failures++; if (failures <= 20) std::printf("line %d: %s\n", __LINE__, #cond); } \
    } while (0)

static MoeFacts mixtral(int T)
{
    MoeFacts f;
    f.T = T; f.experts = 8; f.top_k = 2; f.dim = 4096; f.ffn = 14336; f.w_dtype = 7; f.w_ax8 = 1; f.w_q4 = 1; f.full_quant_gemv = 1; f.norm_kind = 0;
    f.gate_f16 = 1; f.gate_cols_match = 1; f.has_ffn_norm = 1; f.experts_uniform = 1; f.have_table = f.have_table_aos = f.have_table_mo = 1;
    f.rows_use_mfma = f.rows_mfma_ok = f.rows_q4_ok = f.singles_ok = 1; f.caller_norm = 1;
    return f;
}

int main()
{
    static_assert(MOE_N_FACTS == 28 && MOE_N_OUT == 14, "array sizes of ifa_moe_plan");
    {
        const MoePlan p = plan_moe_layer(mixtral(8));      // a batched decode step of 8 queries
        EXPECT(p.kind == MOE_DEVICE_SINGLES && p.router == MOE_ROUTER_FUSED && p.device_ok == 1 && p.cap == 16 && p.tile_rows == 64 && p.small_max == 8);
        EXPECT(p.max_tiles == 0 && p.max_singles == 8 && p.max_smalls == 8 && p.rows_kernel == 1 && p.rows_mfma == 1 && p.smalls_mo == 1);
        EXPECT(p.side_stream == 1 && p.host_sync == 0);
        const MoePlan q = plan_moe_layer(mixtral(384));    // a prompt: 96 rows per expert on average
        EXPECT(q.kind == MOE_DEVICE_GROUPED && q.router == MOE_ROUTER_OPS && q.cap == 768 && q.tile_rows == 128 && q.max_tiles == 14 && q.small_max == 0);
        const MoePlan one = plan_moe_layer(mixtral(1));
        EXPECT(one.kind == MOE_HOST && one.router == MOE_ROUTER_FUSED && one.host_sync == 1 && one.cap == 2 && one.tile_rows == 0 && one.max_singles == 0);
    }
    long plans = 0;
    const int Es[] = {4, 8, 64}, Ks[] = {1, 2, 8};
    for (int E : Es)
        for (int K : Ks)
            for (int bits = 0; bits < (1 << 13); bits++) {
                MoeFacts f = mixtral(1);
                f.experts = E; f.top_k = K;
                int *sw[13] = {&f.moe_device, &f.moe_router_fused, &f.moe_singles, &f.moe_overlap, &f.gemm_rows, &f.rows_mo, &f.have_table,
                               &f.have_table_aos, &f.have_table_mo, &f.rows_use_mfma, &f.rows_mfma_ok, &f.rows_q4_ok, &f.singles_ok};
                for (int b = 0; b < 13; b++) *sw[b] = (bits >> b) & 1;
                for (int T = 1; T <= 512; T++) {
                    f.T = T; f.caller_norm = T & 1;
                    const MoePlan p = plan_moe_layer(f);
                    plans++;
                    EXPECT(p.max_smalls <= E && p.max_singles <= E && p.cap == T * K);
                    EXPECT(!p.smalls_mo || p.rows_mfma);
                    EXPECT(!p.smalls_mo || (p.rows_kernel && p.max_smalls > 0));
                    EXPECT(!p.side_stream || p.kind == MOE_DEVICE_SINGLES);
                    EXPECT(p.host_sync == (p.kind == MOE_HOST));
                    EXPECT(p.kind != MOE_DEVICE_SINGLES || p.max_tiles == 0);
                    EXPECT(p.kind != MOE_HOST || (p.tile_rows == 0 && p.max_tiles == 0 && p.max_singles == 0 && p.max_smalls == 0 && !p.side_stream));
                    EXPECT(p.kind == MOE_HOST || (p.device_ok && T > 1 && (p.tile_rows == 64 || p.tile_rows == 128)));
                    EXPECT(p.kind == MOE_HOST || p.max_tiles == 0 || p.max_tiles * p.tile_rows >= p.cap);      // the tile list holds every pair
                    EXPECT((p.small_max == 8) == (p.rows_kernel == 1) && (p.small_max == 0) == (p.rows_kernel == 0));
                    EXPECT(p.router == MOE_ROUTER_OPS || T == 1 || (p.kind != MOE_HOST && T <= 32 && f.caller_norm));
                }
            }
    std::printf("%ld plans, %d failures\n", plans, failures);
    return failures ? 1 : 0;
}
