// lookup_draft.h -- where the draft tokens of lookup decoding come from (InferenceEngine::GenerateLookup), as a pure host function:
// the continuation of the longest recent n-gram, looked up first in a caller-supplied prediction of the output ("predicted outputs"
// of an edit / rewrite request) and then in the query's own tokens (prompt-lookup decoding).  No device calls; the C ABI exposes it
// for tests (ifa_lookup_draft).
#pragma once

namespace inferflow_amd {

// For g = ngram_max down to ngram_min (skipped while n_ctx < g): key = the last g tokens of ctx;
//  1. prediction: the LOWEST start j with pred[j .. j + g) == key and j + g < n_pred -> draft = pred[j + g ..);
//  2. else context: the HIGHEST start j < n_ctx - g with ctx[j .. j + g) == key      -> draft = ctx[j + g ..);
// the first g with a match wins; the draft is cut to k tokens and to the end of its source.  Returns the draft length 0..k
// (0: no match at any g), -1 on bad arguments (null ctx / draft_out, null pred with n_pred > 0, negative lengths, k < 1,
// ngram_min < 1, ngram_max < ngram_min).
int LookupDraft(const int *ctx, int n_ctx, const int *pred, int n_pred, int ngram_max, int ngram_min, int k, int *draft_out);

} // namespace inferflow_amd
