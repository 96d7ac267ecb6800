"""bench.py's multi-process path on CPU: world_size 2 over gloo (the GPU run uses the same zokrates_amd.parallel code
with backend nccl = RCCL).  Independent proofs per rank, no data-path collective."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def test_two_ranks_gloo():
    world, steps = 2, 3
    procs = []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT="29533")
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "mp_worker.py"), str(steps)], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=600) for p in procs]
    for p, (out, err) in zip(procs, outs):
        assert p.returncode == 0, err[-2000:]
    line = json.loads(outs[0][0].strip().splitlines()[-1])
    assert line["n_gpus"] == 2 and line["steps"] == steps and line["scaling"] == "weak"
    assert line["ranks_ok"] == 2.0                      # every rank's proofs equal the oracle's
    assert line["sharded_ok"] == 2.0                    # the proof sharded over both ranks equals the oracle's on both
    assert line["sharded_gm17_ok"] == 2.0               # and so does the GM17 proof
    assert line["sharded_bound_split_ok"] == 2.0        # bound shards with the witness map split between the ranks: the same proof
    assert line["distinct_witnesses_per_rank"] == steps
    assert line["seed_sum"] == 2 * 0x5EED0000 + 1000    # ranks drew different witness seeds
    assert line["value"] > 0
    assert not any(l.startswith("{") for l in outs[1][0].splitlines())   # only rank 0 prints the result line


def launch(world, port, mode, extra_env=None, timeout=300):
    procs = []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.update(extra_env or {})
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "mp_worker.py"), "1", mode], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    try:
        outs = [p.communicate(timeout=timeout) for p in procs]      # (a rank waiting for a partner that never comes: a failure here, not a hang)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, (out, err) in zip(procs, outs):
        assert p.returncode == 0, err[-2000:]
    return json.loads(outs[0][0].strip().splitlines()[-1])


def test_three_ranks_bound_split_the_odd_rank_out():
    """World 3, bound shards, transform_split=True: ranks 0 and 1 swap halves, rank 2 — without a partner of its own — receives rank 1's
    partner's half from rank 1 (parallel.prove_sharded), over a real process group."""
    line = launch(3, 29563, "odd_rank_out")
    assert line["n_gpus"] == 3 and line["bound_ranks"] == 3.0
    assert line["sharded_bound_split_ok"] == 3
    assert line["afterwards_ok"] == 3.0


def test_two_ranks_one_unbound_agree_not_to_split():
    """World 2, rank 1 skipped bind_shard, transform_split=None with the threshold at 2^0: rank 0 alone would split and wait for a
    half that rank 1 — on its way to the all-gather — never sends.  The ranks agree first (MIN over the ranks): nobody splits, and —
    a bound shard's record and an unbound shard's do not add up to the proof — rank 0 gives its binding up; both return the oracle's
    proof."""
    line = launch(2, 29567, "one_rank_unbound", {"ZKHIP_SPLIT_MIN_LOG": "0"})
    assert line["n_gpus"] == 2 and line["bound_ranks"] == 0.0      # (one rank was bound before the call: the worker asserts it)
    assert line["sharded_bound_split_ok"] == 2.0
    assert line["afterwards_ok"] == 2.0
