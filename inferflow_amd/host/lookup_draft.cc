// lookup_draft.cc -- see lookup_draft.h
#include "lookup_draft.h"

#include <algorithm>

namespace inferflow_amd {

static bool same(const int *a, const int *b, int n)
{
    for (int i = 0; i < n; i++) if (a[i] != b[i]) return false;
    return true;
}

int LookupDraft(const int *ctx, int n_ctx, const int *pred, int n_pred, int ngram_max, int ngram_min, int k, int *draft_out)
{
    if (!ctx || !draft_out || n_ctx < 0 || n_pred < 0 || (n_pred > 0 && !pred) || k < 1 || ngram_min < 1 || ngram_max < ngram_min) return -1;
    for (int g = ngram_max; g >= ngram_min; g--) {
        if (n_ctx < g) continue;
        const int *key = ctx + (n_ctx - g);
        const int *src = nullptr;
        int n_src = 0;
        for (int j = 0; j + g < n_pred && !src; j++)
            if (same(pred + j, key, g)) { src = pred + j + g; n_src = n_pred - (j + g); }
        for (int j = n_ctx - g - 1; j >= 0 && !src; j--)      // (j + g < n_ctx: the continuation holds at least one token)
            if (same(ctx + j, key, g)) { src = ctx + j + g; n_src = n_ctx - (j + g); }
        if (!src) continue;
        const int n = std::min(k, n_src);
        for (int i = 0; i < n; i++) draft_out[i] = src[i];
        return n;
    }
    return 0;
}

} // namespace inferflow_amd
