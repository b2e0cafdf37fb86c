"""The search on the MI355X: gzpx_find_device against what it rides on and what it replaces.  Two inputs, each compressed
at level 1 on the device as BGZF and resident in HBM: bench.py's 550 MiB text slab, and 550 MiB of
gzpx_synth_fastq_device output.  One process, warm, median / min / max of the steps.  Four patterns per input, chosen
from the input itself: a 12-byte slice with on the order of 1,000 hits (`rare`), the same with its last byte replaced so
that it never matches (`absent`), "\\n" (`dense`), and the input's most frequent byte, its most frequent successor and two
bytes its first 64 MiB do not hold (`frequent_first_byte`).  Every row records its hit count.

  1  the counting pass (count + scan kernels, HIP events, summed over the batches) next to a device-to-device copy of the
     same inflated bytes and next to k_ln_count of a line-table build
  2  find_device, a count-only call and then a writing call (positions and lines, hits_cap = n_hits), host clock,
     synchronised, against the detour: decompress_stream_device of everything + a copy into pinned host memory (timed
     once a step, shared by the step's four patterns) + bytes.find in a loop (timed per pattern); and next to plain
     decompress_stream_device

Prints one JSON line; --out FILE writes it too.

    python tools/find_measure.py [--steps 10] [--warmup 2] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from gzp_amd import _native, build, synth  # noqa: E402


def stats(ms):
    return {"median": round(float(np.median(ms)), 4), "min": round(float(min(ms)), 4), "max": round(float(max(ms)), 4)}


def host_find(buf, pattern):
    hits, p = 0, buf.find(pattern)
    while p >= 0:
        hits += 1
        p = buf.find(pattern, p + 1)
    return hits


def choose_patterns(host):
    """From the first 64 MiB: the 12-byte slice (no newline in it) whose count is nearest to 1,000 over the whole input."""
    head = host[:64 << 20].tobytes()
    scale = host.size / len(head)
    rng = np.random.default_rng(20260201)
    best, best_err = None, None
    for at in rng.integers(0, len(head) - 12, 48).tolist():
        cand = head[at:at + 12]
        if b"\n" in cand:
            continue
        err = abs(np.log(max(head.count(cand), 1) * scale / 1000.0))
        if best is None or err < best_err:
            best, best_err = cand, err
    absent_byte = next(b for b in range(1, 256) if bytes([b]) not in head)
    a = np.frombuffer(head[:16 << 20], dtype=np.uint8)
    f = int(np.bincount(a, minlength=256).argmax())
    g = int(np.bincount(a[1:][a[:-1] == f], minlength=256).argmax())
    return {"absent": best[:11] + bytes([absent_byte]), "rare": best, "dense": b"\n",
            "frequent_first_byte": bytes([f, g, absent_byte, absent_byte])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bytes", type=int, default=576_716_800)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    n = args.bytes
    res = {"what": "find_measure", "build_id": build.source_id(), "device": torch.cuda.get_device_name(0), "bytes": n,
           "steps": args.steps, "warmup": args.warmup, "inputs": {}}

    def clock(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    d_in = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    d_full = torch.empty(n + 64, dtype=torch.uint8, device="cuda:0")
    d_copy = torch.empty(n + 64, dtype=torch.uint8, device="cuda:0")
    h_full = torch.empty(n, dtype=torch.uint8).pin_memory()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for which in ("text_slab", "fastq"):
        if which == "text_slab":
            d_in.copy_(torch.from_numpy(synth.text_slab(n, seed=20250927)))
        else:
            _native.synth_fastq_device(d_in.data_ptr(), 0, n)
        torch.cuda.synchronize()
        with _native.Context(format=_native.FORMAT_BGZF, level=1, buffer_size=65280, max_slab_bytes=n) as c:
            cap = c.slab_bound(n)
            d_comp = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
            comp_len, _ = c.compress_slab_device(d_in.data_ptr(), n, d_comp.data_ptr(), cap, True)
        p_comp = d_comp.data_ptr()
        patterns = choose_patterns(d_in.cpu().numpy())
        one = {"compressed_bytes": int(comp_len), "patterns": {k: v.hex() for k, v in patterns.items()}, "rows": {}}
        with _native.DContext(format=_native.FORMAT_BGZF) as d, d.build_index_device(p_comp, comp_len) as ix:
            one["members"] = ix.n_members
            hits = {k: d.find_device(ix, p_comp, comp_len, v) for k, v in patterns.items()}
            room = max(max(hits.values()), 1)
            d_pos = torch.empty(room, dtype=torch.int64, device="cuda:0")
            d_lines = torch.empty(room, dtype=torch.int64, device="cuda:0")
            rows = {k: {"count_call": [], "write_call": [], "count_pass": [], "write_pass": [], "inflate": [], "host_find": [],
                        "detour": []} for k in patterns}
            shared = {"inflate_copy": [], "plain": [], "d2d": [], "k_ln_count": []}
            host_hits = {}
            for step in range(args.warmup + args.steps):
                keep = step >= args.warmup
                t_ic = clock(lambda: (d.decompress_stream_device(p_comp, comp_len, d_full.data_ptr(), n + 64), h_full.copy_(d_full[:n])))
                t_p = clock(lambda: d.decompress_stream_device(p_comp, comp_len, d_full.data_ptr(), n + 64))
                ev0.record()
                d_copy[:n].copy_(d_full[:n], non_blocking=True)
                ev1.record()
                ev1.synchronize()
                d.build_lines_device(ix, p_comp, comp_len).close()
                ln_count = d.last_lines_build_ms()[1]
                if keep:
                    shared["inflate_copy"].append(t_ic)
                    shared["plain"].append(t_p)
                    shared["d2d"].append(ev0.elapsed_time(ev1))
                    shared["k_ln_count"].append(ln_count)
                buf = memoryview(h_full.numpy()).tobytes() if step == 0 else buf  # (bytes.find needs bytes: made once, outside the clock)
                for k, pat in patterns.items():
                    t0 = time.perf_counter()
                    host_hits[k] = host_find(buf, pat)
                    t_f = (time.perf_counter() - t0) * 1e3
                    t_c = clock(lambda: d.find_device(ix, p_comp, comp_len, pat))
                    count_pass = d.last_find_ms()[1]
                    got = []
                    t_w = clock(lambda: got.append(d.find_device(ix, p_comp, comp_len, pat, 10, d_pos.data_ptr(), d_lines.data_ptr(), hits[k])))
                    ms = d.last_find_ms()
                    assert got[0] == hits[k] == host_hits[k], (which, k, got, hits[k], host_hits[k])
                    if keep:
                        r = rows[k]
                        r["count_call"].append(t_c)
                        r["write_call"].append(t_w)
                        r["count_pass"].append(count_pass)
                        r["write_pass"].append(ms[2])
                        r["inflate"].append(ms[0])
                        r["host_find"].append(t_f)
                        r["detour"].append(t_ic + t_f)
            d2d = stats(shared["d2d"])
            one["shared"] = {"d2d_copy_same_bytes_ms": d2d, "k_ln_count_ms": stats(shared["k_ln_count"]),
                             "detour_inflate_copy_ms": stats(shared["inflate_copy"]), "plain_stream_device_ms": stats(shared["plain"])}
            for k, r in rows.items():
                both = [a + b for a, b in zip(r["count_call"], r["write_call"])]
                cp = stats(r["count_pass"])
                one["rows"][k] = {
                    "pattern_bytes": len(patterns[k]), "hits": int(hits[k]),
                    "run1": {"counting_pass_ms": cp, "GB_per_s": round(n / (cp["median"] / 1e3) / 1e9, 1) if cp["median"] > 0 else 0.0,
                             "not_slower_than_copy": bool(cp["median"] <= d2d["median"])},
                    "run2": {"find_count_call_ms": stats(r["count_call"]), "find_write_call_ms": stats(r["write_call"]),
                             "find_both_calls_ms": stats(both), "inflate_kernels_ms": stats(r["inflate"]),
                             "writing_pass_ms": stats(r["write_pass"]), "host_bytes_find_ms": stats(r["host_find"]),
                             "detour_ms": stats(r["detour"]), "find_max_lt_detour_min": bool(max(both) < min(r["detour"])),
                             "count_call_over_plain_ms": round(float(np.median(r["count_call"]) - np.median(shared["plain"])), 4)}}
            # the writing call's answer against the slab, once, behind the timers: the rare pattern's positions and lines
            k = "rare"
            assert d.find_device(ix, p_comp, comp_len, patterns[k], 10, d_pos.data_ptr(), d_lines.data_ptr(), hits[k]) == hits[k]
            pos = d_pos[:hits[k]].cpu().numpy()
            a = np.frombuffer(buf, dtype=np.uint8)
            assert all(buf[p:p + 12] == patterns[k] for p in pos.tolist()) and bool(np.all(np.diff(pos) > 0))
            nl = np.flatnonzero(a == 10)
            assert np.array_equal(d_lines[:hits[k]].cpu().numpy(), np.searchsorted(nl, pos, side="left"))
            del buf, a, nl
        res["inputs"][which] = one
        del d_comp, d_pos, d_lines
    res["note"] = ("calls, detour, plain: host clock around work that is synchronised at both ends; counting_pass (count + scan), "
                   "writing_pass (write + carry), inflate_kernels, k_ln_count and d2d: HIP events, summed over the batches.  "
                   "detour = this step's inflate + copy to pinned memory, timed once and shared by the step's patterns, + this "
                   "pattern's bytes.find loop.  GB/s count the inflated bytes once.")
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
