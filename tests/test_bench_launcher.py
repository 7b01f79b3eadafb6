"""bench.py's N-rank entry, on the CPU: `--gpus N` without a torchrun wrapper starts the N
ranks itself and relays rank 0's line, refuses to run with fewer GPUs than asked, and kills ranks that pass its
deadline.  The rank bodies here are the gloo `--launcher-check` (no GPU, no HIP library); the GPU rehearsal of
the real step (`CC_BENCH_ONE_DEVICE=1 python bench.py --gpus 2`) is in tests/test_gpu_sharded.py.  Also here: the
host logic of `--dump-outputs`, and one plain single-GPU run (small shapes) with its dump."""
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def run(args, env_extra=None, timeout=240):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra or {})
    env["PYTHONDONTWRITEBYTECODE"] = "1"
    t0 = time.monotonic()
    p = subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, env=env, timeout=timeout,
                       cwd=ROOT)
    return p, time.monotonic() - t0


def json_lines(out):
    return [json.loads(s) for s in out.splitlines() if s.startswith("{")]


def test_gpus_2_launches_two_ranks_without_torchrun():
    p, _ = run(["--gpus", "2", "--launcher-check"])
    assert p.returncode == 0, p.stderr[-2000:]
    lines = json_lines(p.stdout)
    assert len(lines) == 1, p.stdout
    assert lines[0]["n_gpus"] == 2 and lines[0]["world_size_pg"] == 2
    assert lines[0]["rank_sum"] == 1.0  # ranks 0 + 1 took part in the collective


def test_gpus_more_than_visible_exits_nonzero_without_a_line():
    import torch

    n = max(8, torch.cuda.device_count() + 1)
    p, _ = run(["--gpus", str(n)])
    assert p.returncode != 0
    assert json_lines(p.stdout) == []
    assert "visible GPUs" in p.stderr


def test_world_size_mismatch_exits_nonzero():
    p, _ = run(["--gpus", "4", "--launcher-check"], env_extra={"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert p.returncode == 2
    assert json_lines(p.stdout) == []


def test_deadline_kills_a_hung_rank():
    p, dt = run(["--gpus", "2", "--launcher-check", "hang", "--deadline", "25"], timeout=200)
    assert p.returncode == 124, (p.returncode, p.stderr[-2000:])
    assert dt < 120
    assert "deadline" in p.stderr


@pytest.mark.parametrize("n", [3])
def test_gpus_n_relays_rank0_line(n):
    p, _ = run(["--gpus", str(n), "--launcher-check"])
    assert p.returncode == 0, p.stderr[-2000:]
    (line,) = json_lines(p.stdout)
    assert line["n_gpus"] == n and line["rank_sum"] == float(sum(range(n)))


def test_effective_clock_from_tile_sum_words():
    """bench.py's clock report: shader-clock ticks over 100 MHz wall ticks (gemm.hip WgradTail::clock layout:
    [sclk ticks, wall ticks, launches, ...]); no launch recorded gives no report."""
    import importlib.util
    import torch
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    words = torch.zeros(8, dtype=torch.int64)
    assert bench.effective_clock(words) is None
    words[0], words[1], words[2] = 1_720_000_000, 100_000_000, 3     # 1 s of wall ticks at 1.72 GHz
    rep = bench.effective_clock(words)
    assert rep["effective_sclk_ghz"] == pytest.approx(1.72)
    assert rep["launches"] == 3 and rep["window_ms"] == pytest.approx(1000.0)
    assert bench.effective_clock(None) is None


def _load_bench():
    import importlib.util

    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_dump_outputs_writes_losses_and_seeded_parameter_samples(tmp_path):
    """bench.py --dump-outputs, its host logic: losses.npy is the step's loss dict in LOSS_KEYS order (float64); each
    parameter is written flattened as float32, whole when it has at most DUMP_SAMPLE elements, else the elements at
    DUMP_SAMPLE seeded indices -- the same ones in every call."""
    import numpy as np
    import torch

    bench = _load_bench()
    bench.DUMP_SAMPLE = 64
    sd = {"W_enc": torch.arange(2 * 8 * 32, dtype=torch.float32).reshape(2, 8, 32).to(torch.bfloat16),
          "W_dec": -torch.arange(32 * 2 * 8, dtype=torch.float32).reshape(32, 2, 8).to(torch.bfloat16),
          "b_enc": torch.linspace(0, 1, 32).to(torch.bfloat16), "b_dec": torch.ones(2, 8, dtype=torch.bfloat16)}
    calls = []
    tr = type("T", (), {"synchronize": lambda self: calls.append("sync")})()
    tr.crosscoder = type("C", (), {"state_dict": lambda self: dict(sd)})()
    last = {k: 0.5 + i for i, k in enumerate(bench.LOSS_KEYS)}
    out = [tmp_path / "a", tmp_path / "b" / "nested"]
    for o in out:
        bench.dump_outputs(str(o), tr, last)
    assert calls == ["sync", "sync"]
    got = [{f[:-4]: np.load(o / f) for f in sorted(os.listdir(o))} for o in out]
    assert sorted(got[0]) == ["W_dec", "W_enc", "b_dec", "b_enc", "losses"]
    for k, v in got[0].items():
        assert v.dtype == (np.float64 if k == "losses" else np.float32) and v.ndim == 1, k
        assert np.array_equal(v, got[1][k]), k
    assert got[0]["losses"].tolist() == [0.5 + i for i in range(9)]
    assert np.array_equal(got[0]["b_enc"], sd["b_enc"].float().numpy())
    assert np.array_equal(got[0]["b_dec"], np.ones(16, dtype=np.float32))
    for k in ("W_enc", "W_dec"):  # 512 elements: sampled; every value names its own index (exact in bf16 below 256,
        flat = sd[k].float().reshape(-1).numpy()  # so compare by membership and count)
        assert got[0][k].shape == (64,) and np.isin(got[0][k], flat).all()
        assert len(np.unique(got[0][k])) > 16
    assert not np.array_equal(np.abs(got[0]["W_enc"]), np.abs(got[0]["W_dec"]))  # (one generator, drawn in order)


def test_plain_and_full_options_parse():
    """`--full` and `--dump-outputs DIR` exist and default to off; a run with no timed step is refused."""
    p, _ = run(["--steps", "0"])
    assert p.returncode == 2 and "--steps" in p.stderr
    p, _ = run(["--help"])
    assert p.returncode == 0 and "--full" in p.stdout and "--dump-outputs DIR" in p.stdout


@pytest.mark.gpu
def test_plain_run_prints_the_headline_line_and_dumps_its_outputs(gpu, tmp_path):
    """A plain `bench.py --gpus 1` run (small shapes) prints one line with the headline fields and none of the
    `--full` measurements, and `--dump-outputs` writes the last timed step's losses and the updated parameters."""
    import numpy as np

    out = tmp_path / "dump"
    p, _ = run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "256", "--d-model", "64", "--dict-size",
                "512", "--dump-outputs", str(out)])
    assert p.returncode == 0, p.stderr[-3000:]
    (line,) = json_lines(p.stdout)
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "activations/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
    # (ms_per_step is rounded to 1e-4 ms: under 0.5 % of any step above 0.02 ms)
    assert line["ms_per_step"] > 0.02 and line["value"] == pytest.approx(256 / (line["ms_per_step"] * 1e-3), rel=5e-3)
    assert not {"kernels_ms", "roofline", "hbm", "cpu_baseline", "n1_same_workload"} & set(line)
    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert {k: v.shape for k, v in got.items()} == {"losses": (9,), "W_enc": (2 * 64 * 512,), "W_dec": (512 * 2 * 64,),
                                                    "b_enc": (512,), "b_dec": (2 * 64,)}
    bench = _load_bench()
    for v, k in zip(got["losses"], bench.LOSS_KEYS):
        assert v == pytest.approx(line["last_loss"][k], abs=1e-6), k
    for k, v in got.items():
        assert v.dtype == (np.float64 if k == "losses" else np.float32) and np.isfinite(v).all(), k
    assert np.abs(got["b_enc"]).max() > 0  # (b_enc starts at zero: the dump is taken after the Adam updates)


class _FakeShardedTrainer:
    """ShardedTrainer's surface measure_exchange uses (engine.comm, backend.row_chunks, step), with a step whose time
    depends on the exchange form (reduce_scatter slower on rank 1: every rank must still pick the same form)."""

    def __init__(self, rank):
        import torch.distributed as dist

        self.rank, self.dist = rank, dist
        self.engine = type("E", (), {"comm": "all_reduce"})()
        bk = self.backend = type("Bk", (), {"recon_chunks": 2})()
        bk.row_chunks = lambda: [(r0, r0 + 32 // bk.recon_chunks) for r0 in range(0, 32, 32 // bk.recon_chunks)]
        self.comms = []

    def step(self):
        import torch

        self.comms.append((self.engine.comm, self.backend.recon_chunks))
        ar = 0.002 if self.backend.recon_chunks == 2 else 0.004 + 0.002 * self.rank
        time.sleep(ar if self.engine.comm == "all_reduce" else 0.006 + 0.004 * self.rank)
        t = torch.ones(4)
        self.dist.all_reduce(t)


def _exchange_rank(rank, world, port, q):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        bench = _load_bench()
        tr = _FakeShardedTrainer(rank)
        ex = bench.measure_exchange(tr, "auto", K=8, dev="cpu", steps=3)
        kern = {"G1_encode": 0.5, "exchange_wait0": 0.12, "exchange_wait1": 0.01, "sums_allreduce": 0.02}
        bench.exchange_exposed(kern, ex)
        q.put((rank, ex, kern, (tr.engine.comm, tr.backend.recon_chunks), sorted(set(tr.comms))))
    finally:
        dist.destroy_process_group()


def test_sharded_bench_exchange_fields_over_two_gloo_ranks():
    """The N > 1 line's exchange evidence, its host logic over 2 gloo ranks: the exchange
    forms (the all-reduce in 1, 2 and 4 batch slices, the reduce-scatter) are timed in warm-up (max over ranks), the
    fastest is left set on the trainer -- the same on every rank --,
    one slice's all-reduce bandwidth is measured, and the attribution pass's exchange spans become the exposed time
    per step (removed from the kernel table)."""
    import random

    import torch.multiprocessing as mp

    world, port = 2, 27000 + random.randint(0, 900)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_exchange_rank, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict((r[0], r[1:]) for r in (q.get(timeout=120) for _ in range(world)))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank in range(world):
        ex, kern, comm, tried = res[rank]
        assert tried == [("all_reduce", 1), ("all_reduce", 2), ("all_reduce", 4), ("reduce_scatter", 2)]
        assert comm == ("all_reduce", 2) and ex["comm"] == "all_reduce"
        assert set(ex) == {"comm", "chosen_by", "trial_ms_per_step", "slices", "slice_allreduce",
                           "exposed_ms_per_step", "exposed_ms_by_slice", "sums_allreduce_ms"}
        tr_ms = ex["trial_ms_per_step"]
        assert set(tr_ms) == {"all_reduce x1", "all_reduce x2", "all_reduce x4", "reduce_scatter"}
        assert min(tr_ms["reduce_scatter"], tr_ms["all_reduce x1"], tr_ms["all_reduce x4"]) > tr_ms["all_reduce x2"] > 0
        assert ex["slices"] == 2 and ex["slice_allreduce"]["bytes"] == 16 * 8 * 4
        assert ex["slice_allreduce"]["busbw_GB_s"] == pytest.approx(ex["slice_allreduce"]["algbw_GB_s"], rel=0.01)
        assert ex["exposed_ms_per_step"] == pytest.approx(0.13) and ex["sums_allreduce_ms"] == 0.02
        assert ex["exposed_ms_by_slice"] == {"0": 0.12, "1": 0.01}
        assert kern == {"G1_encode": 0.5}
    # (the forms' times are all-reduced: both ranks report the same trial table)
    assert res[0][0]["trial_ms_per_step"] == res[1][0]["trial_ms_per_step"]
