"""-m gpu: bench.py's contract on one GPU -- ONE JSON line on stdout whatever RCCL prints, the multi-GPU fallback chain
(C path with the captured step -> C path with eager steps -> torch.distributed runner) with injected failures, and the
single-device loopback mode.  Small step counts: this checks the plumbing, not the numbers."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra_env, *args):
    env = dict(os.environ, **extra_env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--no-cpu-baseline", "--prefill-lens", "", "--batch", "0",
                        "--steps", "8", "--warmup", "2", "--shape", "test_gqa"] + list(args), capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[-2000:]                   # exactly one line on stdout
    return json.loads(lines[0]), r.stderr


def test_single_gpu_line_has_the_contract_keys():
    j, _ = _run({})
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in j, k
    assert j["n_gpus"] == 1 and j["steps"] == 8 and j["value"] > 0 and j["config"]["fallbacks"] == []
    assert "roofline" not in j and "kernels" not in j and "decode_tok_s_by_context" not in j     # --full legs only


def test_full_adds_the_legs_of_their_own():
    j, _ = _run({}, "--full")
    assert j["value"] > 0 and j["roofline"]["achieved"] > 0 and set(j["kernels"]) == {"qkv", "attn", "wo", "ffn13", "w2", "lm_head"}
    assert list(j["prefill_tok_s_by_prompt_len"]) == ["16"]        # (--prefill-lens "": the prompt's own length only)


def test_dump_outputs_are_what_the_timed_call_returned(tmp_path):
    """--dump-outputs: the ids of the timed steps and the logits row of the last step (the id it chose is a maximum of it)."""
    import numpy as np
    j, _ = _run({}, "--dump-outputs", str(tmp_path))
    toks, logits = np.load(tmp_path / "tokens.npy"), np.load(tmp_path / "logits.npy")
    assert toks.dtype == np.float64 and logits.dtype == np.float32
    assert toks.shape == (8,) and [int(t) for t in toks[-4:]] == j["last_tokens"]
    assert logits.ndim == 1 and np.isfinite(logits).all() and logits[int(toks[-1])] == logits.max()
    _run({}, "--dump-outputs", str(tmp_path / "again"))
    assert np.array_equal(np.load(tmp_path / "again" / "tokens.npy"), toks)                # same arguments, same inputs
    assert np.array_equal(np.load(tmp_path / "again" / "logits.npy"), logits)


@pytest.mark.parametrize("inject,expect", [("", "c-abi"), ("c-graph", "[eager steps]"), ("c-graph,c-eager", "torch.distributed")])
def test_forced_collectives_and_the_fallback_chain(inject, expect):
    """IFA_FORCE_TP=1 makes a one-rank job issue every collective of the multi-GPU step; IFA_BENCH_FAIL_MODES injects a failure
    into the named modes: the line must come from the next mode and list what failed."""
    env = {"IFA_FORCE_TP": "1", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "29541", "RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0"}
    if inject:
        env["IFA_BENCH_FAIL_MODES"] = inject
    j, err = _run(env)
    assert expect in j["config"]["collectives"], j["config"]
    assert [f["mode"] for f in j["config"]["fallbacks"]] == [m for m in inject.split(",") if m]
    assert j["value"] > 0


def test_loopback_two_ranks_on_one_device():
    env = dict(os.environ)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--loopback", "2", "--steps", "8", "--warmup", "2", "--shape", "test_gqa"],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert "tp2 loopback" in j["config"]["parallelism"] and "partition_ranks = 2" in j["config"]["parallelism"] and j["value"] > 0
