"""bench.py's harness contract: the N-GPU launch rules and the config loop (CPU checks), and what
a plain run reports and dumps (GPU tests)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                          timeout=120, env=env)


def test_world_size_must_match_gpus():
    """Under a launcher that started a different number of ranks than --gpus: a clean
    non-zero exit naming both numbers (no silent 1-rank run labelled n_gpus N)."""
    r = _run(["--gpus", "2"], {"RANK": "0", "WORLD_SIZE": "3", "LOCAL_RANK": "0"})
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert "--gpus 2 but the launcher started 3 ranks" in r.stderr


def test_rccl_needs_one_gpu_per_rank():
    """--gpus N with RCCL on a node with fewer GPUs fails fast before spawning ranks
    (RCCL refuses two ranks on one GPU: profiles/rccl_two_ranks_one_gpu_r2.txt)."""
    import torch

    n = torch.cuda.device_count() + 1
    r = _run(["--gpus", str(n)])
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert "needs" in r.stderr and "GPU" in r.stderr


def test_full_and_dump_outputs_are_options():
    """`--full` (everything beyond the headline figure) and `--dump-outputs DIR` exist; off by default."""
    r = _run(["--help"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--full" in r.stdout and "--dump-outputs DIR" in r.stdout


def _load(d):
    import numpy as np

    return {f[:-4]: np.load(d / f) for f in os.listdir(d) if f.endswith(".npy")}


def _dump_run(out):
    import json

    # (lr 1e-3: the run's few steps are small ones)
    r = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "128", "--hidden", "256", "--nbatches", "2",
              "--lr", "0.001", "--dump-outputs", str(out)])
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1]), _load(out), _load(out / "trajectory")


@pytest.mark.gpu
def test_plain_run_is_headline_only_and_dumps_its_outputs(tmp_path):
    """A plain run times exactly --steps steps, reports ms_per_step and no secondary measurement,
    and --dump-outputs writes finite float32 / float64 arrays:
    * DIR/trajectory: the last timed step as it ran.  Its loss sum covers the warm-up + timed steps:
      bounds on one step's mean loss (see below) leave 1 + 3 as the only number of steps the loop can
      have run, independently of the record's own arithmetic; the record's train_loss is that sum
      per sample; the weights have moved from the one-step ones.
    * DIR/: the same step from the seeded initial weights, the same from run to run: logits and
      statistics bit for bit (the forward and the per-workgroup statistics have one summation
      order), weights and momentum up to the fp32 rounding of the gradient sums whose order varies
      (atomics): a few ulp, bounds 4 x 2^-24 of max|weight| and 16 x 2^-24 of max|momentum| --
      ten times the 0.4 / 1.7 x 2^-24 measured on the headline config (batch 16384, hidden 4096);
      this config measured 0."""
    import numpy as np

    rec, arrs, traj = _dump_run(tmp_path / "a")
    assert rec["steps"] == 3 and rec["ms_per_step"] > 0 and "configs" not in rec
    assert abs(rec["value"] - 128 / rec["ms_per_step"] * 1e3) <= 1e-2 * rec["value"]
    for k in ("metric", "unit", "higher_is_better", "dtype"):
        assert k in rec
    names = {"logits", "loss_stats", "weights_sample", "momentum_sample"}
    assert set(arrs) == names | {"sample_index"} and set(traj) == names
    for d in (arrs, traj):
        assert d["logits"].shape == (128, 10) and d["loss_stats"].shape == (2,)
        assert d["weights_sample"].shape == arrs["sample_index"].shape == d["momentum_sample"].shape
        for a in d.values():
            assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all()
        assert d["weights_sample"].any() and d["momentum_sample"].any() and d["logits"].any()
    # one step of 128 samples from the Xavier start: a mean loss near ln 10 on uniform labels
    assert 1.0 < arrs["loss_stats"][0] / 128 < 4.0 and 0 <= arrs["loss_stats"][1] <= 128
    # the number k of steps behind the trajectory's loss sum, from two bounds on a step's mean loss
    # (uniform random labels, ten or so steps at lr 1e-3): at least 0.95 ln 10 (below ln 10 only by
    # memorising, which so few small steps cannot do by 5 %) and at most 1.05 x the seeded start's
    # (training lowers it; another batch of 128 samples moves the mean by ~2 %)
    l0, lsum = arrs["loss_stats"][0] / 128, traj["loss_stats"][0] / 128
    kmin, kmax = lsum / (1.05 * l0), lsum / (0.95 * np.log(10.0))
    print("start loss", l0, "trajectory loss sum per sample", lsum, "steps in", (kmin, kmax))
    assert 3 < kmin <= 4 <= kmax < 5 and 0 <= traj["loss_stats"][1] <= 4 * 128
    assert abs(rec["train_loss"] - traj["loss_stats"][0] / (4 * 128)) <= 1e-3
    assert not np.array_equal(traj["weights_sample"], arrs["weights_sample"])
    _, again, _ = _dump_run(tmp_path / "b")
    for k in ("logits", "loss_stats", "sample_index"):
        assert np.array_equal(arrs[k], again[k]), k
    for k, ulps in (("weights_sample", 4), ("momentum_sample", 16)):
        d = np.abs(arrs[k].astype(np.float64) - again[k]).max()
        print(k, "max|a-b|", d, "max|a|", np.abs(arrs[k]).max())
        assert d <= ulps * 2.0 ** -24 * np.abs(arrs[k]).max(), (k, d)


@pytest.mark.gpu
def test_plain_two_rank_run_leaves_the_local_step_to_full():
    """N > 1 without --full (two gloo ranks on one GPU): the headline only -- no comm-free local
    engine, so per_gpu_local_ms / scaling_efficiency are null, no comm_us, no configs."""
    import json

    r = _run(["--gpus", "2", "--backend", "gloo", "--steps", "2", "--warmup", "1", "--batch", "128", "--hidden", "256",
              "--nbatches", "2"])
    assert r.returncode == 0, r.stderr[-2000:]
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert rec["n_gpus"] == 2 and rec["steps"] == 2 and rec["ms_per_step"] > 0
    assert rec["per_gpu_local_ms"] is None and rec["scaling_efficiency"] is None
    assert "comm_us" not in rec and "configs" not in rec


def _configs_worker(rank, world, port, q):
    import importlib.util
    import types

    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import datetime

    # (a short timeout: the healthy rank waits inside the failed config's collective until then)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=5))
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    ctx = types.SimpleNamespace(world_size=world, rank=rank, backend="gloo", device="cpu")
    ran = []

    def run_fn(ctx, name, b, st, o):
        ran.append(name)
        if name == "bad" and rank == 1:
            raise RuntimeError("out of memory on rank 1 only")
        if name == "dead" and rank == 0:
            raise RuntimeError("HIP error: an illegal memory access was encountered")
        dist.all_reduce(__import__("torch").ones(1))   # a config's own collectives
        return {"ok": name}

    out = bench.run_configs(ctx, (("a", 1, 1, "sgd"), ("bad", 1, 1, "sgd"), ("c", 1, 1, "sgd")), run_fn)
    q.put((rank, out, list(ran)))
    dist.destroy_process_group()


def test_config_failure_on_one_rank_is_agreed_and_does_not_hang():
    """A secondary config that raises on ONE rank only: the failure flag travels on a side group
    (never paired with the config's own collectives), every rank records the config as failed
    and all ranks stop the config loop together (a lone failing rank sat in a barrier
    while its peers entered the next config's collectives)."""
    import socket

    import torch.multiprocessing as mp

    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_configs_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = dict((r, (o, ran)) for r, o, ran in (q.get(timeout=120) for _ in ps))
    for p in ps:
        p.join(timeout=60)
        assert p.exitcode == 0
    for r in (0, 1):
        out, ran = res[r]
        assert ran == ["a", "bad"]   # both stop after the failed config (the group may be broken)
        assert out["a_b1"] == {"ok": "a"} and "skipped" in out["c_b1"]
        assert "error" in out["bad_b1"]
    assert "out of memory" in res[1][0]["bad_b1"]["error"]
    # rank 0 left the config's own collective at the timeout (its own error), never paired it
    # with rank 1's failure flag
    assert "error" in res[0][0]["bad_b1"]
