"""ifa_attention_mfma_heads is a level, not a flag: 0 off, 1 on, 2 also the batched / draft steps of 256-wide heads
(docs/decode_batch_heads256.md).  It stores and returns 0 / 1 / 2, -1 only queries, the default is 0."""
import inferflow_amd as ia


def test_switch_stores_and_returns_the_level():
    L = ia.lib()
    first = L.ifa_attention_mfma_heads(-1)
    try:
        assert first == 0, "the default level"
        last = first
        for level in (2, 1, 0, 2, 0):
            assert L.ifa_attention_mfma_heads(level) == last, "the call returns the previous level"
            assert L.ifa_attention_mfma_heads(-1) == level and L.ifa_attention_mfma_heads(-1) == level, "-1 queries and changes nothing"
            last = level
    finally:
        L.ifa_attention_mfma_heads(first)
