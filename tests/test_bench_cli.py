"""bench.py's launcher logic (no GPU): `python bench.py --gpus N` without torch.distributed.run around it must start the
launcher as a CHILD process with the same arguments, relay its output and return its exit code - and the parent must not
need a GPU for that (VERDICT r3 missing #1: the first 8-GPU run must not die in argument handling)."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env=None, timeout=300):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + args, capture_output=True, text=True, timeout=timeout, cwd=REPO, env=e)


def test_self_launch_starts_the_launcher_as_a_child_and_relays_its_exit_code(tmp_path):
    """`python bench.py --gpus 2` with no WORLD_SIZE in the environment: the parent must announce and start the launcher command
    (same arguments, 127.0.0.1 rendezvous) as a child process and pass its exit code on. In this container the ranks have no GPU and
    must fail - what is checked is that the PARENT got as far as starting them and relayed the failure instead of dying in argument
    handling; on a GPU box the same call has to produce the one JSON line."""
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0", "--encoder", "vits", "--no-cpu-baseline"], env={"VDA_BENCH_BACKEND": "gloo"})
    assert "[bench] --gpus 2 without a launcher: starting -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1" in r.stderr, r.stderr[-2000:]
    import torch
    if not torch.cuda.is_available():
        assert r.returncode != 0, "ranks without a GPU cannot succeed; the parent must relay that"
        assert "needs torch.distributed.run" not in (r.stdout + r.stderr)
    else:
        line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
        assert r.returncode == 0 and line["n_gpus"] == 2


def test_launcher_world_size_must_match_gpus():
    r = _run(["--gpus", "4", "--steps", "1"], env={"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "started 2 rank(s)" in (r.stdout + r.stderr)


def test_steps_must_be_positive():
    """`ms_per_step` and --dump-outputs (the last timed step's depth) need at least one timed step: rejected before any GPU call."""
    r = _run(["--steps", "0", "--warmup", "0", "--encoder", "vits"])
    assert r.returncode != 0 and "--steps must be at least 1" in r.stderr, r.stderr[-2000:]
