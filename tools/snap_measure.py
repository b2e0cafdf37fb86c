"""Snap on the MI355X: ms per step and MiB/s of bench.py's 550 MiB text slab, device-resident (HIP events around
gzpx_compress_slab_device), the per-kernel times of gzpx_ctx_last_stage_ms and k_snap_chunk's phase clocks; MiB/s host
to host through the twin; and, as the CPU comparison, libsnappy frames over the usable cores (skipped, and said so,
where the binary is not on the machine).  Prints one JSON line; --out FILE writes it too.

    python tools/snap_measure.py [--steps 10] [--warmup 2] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import numpy as np  # noqa: E402

from gzp_amd import _native, build, par, synth  # noqa: E402

MIB = 1 << 20


def device_leg(a, bs, steps, warmup):
    import torch
    with _native.Context(format=_native.FORMAT_SNAP, buffer_size=bs, max_slab_bytes=a.size) as c:
        d_in = torch.from_numpy(a).to("cuda:0")
        cap = c.slab_bound(a.size)
        d_out = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(warmup):
            got, _ = c.compress_slab_device(d_in.data_ptr(), a.size, d_out.data_ptr(), cap, True)
        times = []
        for _ in range(steps):
            ev0.record()
            got, _ = c.compress_slab_device(d_in.data_ptr(), a.size, d_out.data_ptr(), cap, True)
            ev1.record()
            ev1.synchronize()
            times.append(ev0.elapsed_time(ev1))
        c.set_profiling(True)
        c.compress_slab_device(d_in.data_ptr(), a.size, d_out.data_ptr(), cap, True)
        stages = c.last_stage_ms()
        c.set_profiling(False)
        c.debug_snap(True)
        c.compress_slab_device(d_in.data_ptr(), a.size, d_out.data_ptr(), cap, True)
        clocks = c.debug_snap(False)
    ms = float(np.median(times))
    names = ["cycles", "crc", "scan", "extend", "emit", "scan_steps", "copies", "bytes"]
    return {"ms_per_step_median": round(ms, 3), "ms_min": round(min(times), 3), "ms_max": round(max(times), 3),
            "MiB_per_s": round(a.size / MIB / (ms / 1e3), 1), "out_bytes": int(got), "ratio": round(got / a.size, 4),
            "stage_ms": {k: round(v, 3) for k, v in stages.items()},
            "k_snap_chunk_clocks_sum": dict(zip(names, clocks))}


class _Null:
    n = 0

    def write(self, b):
        self.n += len(b)


def twin_leg(a, bs, reps=3):
    best = None
    for _ in range(reps):
        sink = _Null()
        t = time.perf_counter()
        w = par.ParCompressBuilder(par.Snap).buffer_size(bs).num_threads(4).from_writer(sink)
        w.write_chunked(a, 1 << 20)
        w.finish()
        dt = time.perf_counter() - t
        best = dt if best is None else min(best, dt)
    return {"MiB_per_s": round(a.size / MIB / best, 1), "s_best_of_%d" % reps: round(best, 3), "out_bytes": sink.n}


def cpu_leg(a, bs, threads):
    import make_snap_golden as g
    raw = g.load_snappy()
    if raw is None:
        return {"skipped": "no snappy binary on this machine (%s)" % g.SNAPPY_SO}
    from concurrent.futures import ThreadPoolExecutor
    chunks = [a[i:i + 65536].tobytes() for i in range(0, a.size, 65536)]
    t = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        total = sum(len(b) for b in ex.map(raw, chunks))  # (ctypes releases the GIL around the call)
    dt = time.perf_counter() - t
    return {"threads": threads, "MiB_per_s": round(a.size / MIB / dt, 1), "s": round(dt, 3),
            "raw_bytes": total, "note": "raw bodies only (no CRC-32C, no framing): an upper bound of the CPU rate"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bytes", type=int, default=576_716_800)
    ap.add_argument("--buffer-size", type=int, default=131072)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out")
    args = ap.parse_args()
    a = synth.text_slab(args.bytes, seed=20250927)
    res = {"what": "snap_measure", "build_id": build.source_id(), "bytes": a.size, "buffer_size": args.buffer_size,
           "device": device_leg(a, args.buffer_size, args.steps, args.warmup),
           "twin_host_to_host": twin_leg(a, args.buffer_size),
           "cpu_libsnappy": cpu_leg(a, args.buffer_size, args.threads)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
