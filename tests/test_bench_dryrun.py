"""bench.py's control flow without GPUs: `python bench.py --gpus 2` from a bare shell must launch
itself under torch.distributed.run (the driver's 8-GPU run starts it exactly like that), shard the
stream, gather it in order and print ONE JSON line.  --emulate swaps the HIP library for the
CPU-emulated build and RCCL for gloo; nothing is measured."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _run(*extra, full=True, **more_env):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(more_env)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--emulate", "--steps", "1", "--warmup", "1"] +
                       (["--full", "--no-cpu-baseline", "--no-extras"] if full else []) + list(extra), capture_output=True,
                       text=True, timeout=900, env=env, cwd="/tmp")
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_two_ranks_self_launch_ordered_gather():
    d = _run("--gpus", "2", "--slab-bytes", "150000")
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["config"]["slab_bytes"] == 300000
    assert d["config"]["verified_bit_exact_sample"] is True
    for k in ("metric", "value", "unit", "steps", "warmup", "ms_per_step", "higher_is_better", "vs_baseline", "dtype",
              "data", "roofline"):
        assert k in d
    # one run tells the whole story: both in-order write-outs timed back to back, per-rank times in the line
    w = d["writeouts"]
    assert w["value_is"] == "rccl" and w["fastest"] in ("rccl", "offsets")
    assert set(w) == {"rccl", "offsets", "value_is", "fastest"}  # (no IPC window on CPU)
    for m in ("rccl", "offsets"):
        assert len(w[m]["rank_ms_per_step"]) == 2 and len(w[m]["rank_writeout_wait_ms"]) == 2 and w[m]["MiBps"] > 0
        assert d["value_" + m] == w[m]["MiBps"]  # both write-outs at the top level as well
    # the line's value is north_star's write-out, the ordered RCCL gather -- whichever of them is faster (round 5)
    assert abs(w["rccl"]["ms_per_step"] - d["ms_per_step"]) < 1e-6 and d["value"] == d["value_rccl"]
    assert d["config"]["parallelism"].endswith("ordered RCCL gather of the compressed shards to rank 0")
    # ... and the metric's own slab at N ranks: strong scaling, the gathered stream equal to the single-process one
    st = d["strong_550MiB"]
    assert st["slab_bytes"] == 150000 and st["verified_bit_exact_full"] is True and len(st["rank_ms_per_step"]) == 2
    assert d["compat_pinned"] == "1.10" and d["config"]["compat_in_force"].startswith("libdeflate >= 1.1x")


def test_two_ranks_strong_scaling_is_the_value_when_asked_for():
    d = _run("--gpus", "2", "--slab-bytes", "150000", "--scaling", "strong")
    assert d["scaling"] == "strong" and d["value"] == d["strong_550MiB"]["MiBps"]
    assert d["strong_550MiB"]["verified_bit_exact_full"] is True and d["ms_per_step"] == d["strong_550MiB"]["ms_per_step"]


def test_a_hanging_peer_window_leg_does_not_take_the_line_with_it():
    """The IPC-window write-out is the one leg no single-GPU box can rehearse: it runs last and under a watchdog.  Here
    the leg is made to hang on every rank: rank 0 still prints the complete line (RCCL value, strong leg) with
    `peer_error`, every rank ends with exit code 0."""
    d = _run("--gpus", "2", "--slab-bytes", "150000", GZPX_BENCH_TEST_PEER_HANG="1", GZPX_BENCH_PEER_TIMEOUT="3")
    assert "did not finish within 3 s" in d["writeouts"]["peer_error"]
    assert d["value"] == d["value_rccl"] and d["strong_550MiB"]["verified_bit_exact_full"] is True
    assert "peer" not in d["writeouts"] and "value_peer" not in d


def test_eight_ranks_three_blocks():
    """configs[3]'s world size on the CPU: 8 ranks, a slab of three blocks -- five ranks own no block at all and take part
    in every gather with nothing; the strong-scaling leg's gathered stream is still the single-process stream."""
    d = _run("--gpus", "8", "--slab-bytes", "150000")
    assert d["n_gpus"] == 8 and d["value"] == d["value_rccl"] and len(d["writeouts"]["rccl"]["rank_ms_per_step"]) == 8
    st = d["strong_550MiB"]
    assert st["verified_bit_exact_full"] is True and st["shard_bytes_rank0"] == 65280 and len(st["rank_ms_per_step"]) == 8


def test_config4_workload_two_ranks():
    d = _run("--gpus", "2", "--workload", "fastq", "--stream-bytes", "400000")
    c = d["config"]
    assert d["scaling"] == "strong" and c["gpu_inflate_crc_roundtrip_ok"] is True
    assert c["gzip_t_prefix_suffix_rc"] in ([0, 0], None) and c["blocks"] == 7


def test_single_rank_line_has_e2e_and_inflate_legs(capsys, monkeypatch):
    # in-process (no second interpreter): the default line's extra legs
    sys.path.insert(0, ROOT)
    import bench
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--emulate", "--steps", "1", "--warmup", "0", "--full",
                                      "--no-cpu-baseline", "--slab-bytes", "140000"])
    bench.main()
    d = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][0])
    assert d["e2e"]["device_pinned_ok"] and d["e2e"]["api_write_ok"] and d["e2e"]["api_write_64k_ok"]
    assert d["inflate"]["verified_round_trip"] is True and d["inflate"]["roofline"]["kernel"] == "k_inflate_seg"


PLAIN_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config"}


def _dumped(d):
    """--dump-outputs' files: float32 / float64 only, 64 MB at most in all."""
    names = sorted(os.listdir(d))
    assert sum(os.path.getsize(os.path.join(d, f)) for f in names) <= 64 << 20
    out = {f[:-len(".npy")]: np.load(os.path.join(d, f)) for f in names}
    assert all(a.dtype in (np.float32, np.float64) for a in out.values()), {k: a.dtype for k, a in out.items()}
    return out


def _check_dump(out, stream):
    """The dumped arrays against a stream made here: its length, the CRC-32 of every chunk, the sampled bytes."""
    import bench
    n = len(stream)
    assert out["stream_bytes"].tolist() == [n]
    assert out["stream_chunk_crc32"].tolist() == [zlib.crc32(stream[lo:lo + bench.DUMP_CHUNK])
                                                  for lo in range(0, n, bench.DUMP_CHUNK)]
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, n, size=min(n, bench.DUMP_SAMPLE)))
    assert np.array_equal(out["stream_sample"], np.frombuffer(stream, dtype=np.uint8)[idx].astype(np.float32))


def test_plain_run_is_the_headline_alone_and_dumps_its_stream(tmp_path, oracle):
    """No --full: the line carries the headline and nothing measured or checked besides; --steps is the line's step
    count; --dump-outputs writes the last timed step's stream, which is the oracle's stream of the same slab."""
    from gzp_amd import synth
    d = _run("--steps", "3", "--slab-bytes", "140000", "--dump-outputs", str(tmp_path / "out"), full=False)
    assert set(d) == PLAIN_KEYS and d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert d["metric"] == "BGZF compress MiB/s at level 1, 550 MiB text" and d["unit"] == "MiB/s"
    assert d["n_gpus"] == 1 and d["config"]["blocks"] == 3
    out = _dumped(tmp_path / "out")
    assert set(out) == {"stream_bytes", "stream_chunk_crc32", "stream_sample", "block_sizes"}
    want = oracle.compress_stream(synth.text_slab(140000, seed=20250927), oracle.FMT_BGZF, 1, oracle.COMPAT_1_24, 65280)
    _check_dump(out, want)
    assert out["block_sizes"].size == 3 and out["block_sizes"].sum() <= len(want)


def test_two_ranks_plain_run_dumps_the_gathered_stream(tmp_path, oracle):
    """N > 1 without --full: one write-out (rccl), no other legs; rank 0 dumps the whole gathered stream, which is the
    oracle's stream of the ranks' slabs put end to end (every rank compresses its own, seeded by its rank)."""
    from gzp_amd import shard, synth
    d = _run("--gpus", "2", "--slab-bytes", "150000", "--dump-outputs", str(tmp_path / "out"), full=False)
    assert set(d) == PLAIN_KEYS and d["n_gpus"] == 2 and d["scaling"] == "weak" and d["value"] > 0
    out = _dumped(tmp_path / "out")
    assert set(out) == {"stream_bytes", "stream_chunk_crc32", "stream_sample"}
    slab = np.concatenate([synth.text_slab(n, seed=20250927 + r) for r, (lo, n) in enumerate(shard.shard_bytes(300000, 65280, 2))])
    _check_dump(out, oracle.compress_stream(slab, oracle.FMT_BGZF, 1, oracle.COMPAT_1_24, 65280))
