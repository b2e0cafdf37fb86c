"""The search for a set on the MI355X: gzpx_find_set_device against K calls of gzpx_find_device, the route it replaces.
The two inputs of tools/find_measure.py, each compressed at level 1 on the device as BGZF and resident in HBM: bench.py's
550 MiB text slab and 550 MiB of gzpx_synth_fastq_device output.  One process, warm, median / min / max of the steps.
Sets of K = 1, 4, 16, 64 and 256 twelve-byte slices of the input (no newline in them; the K = 1 set is find_measure's
`rare`), and on the FASTQ input one set of 96 eight-byte strings over ACGT (`barcodes`: a 4-byte window passes the
filter nearly everywhere).  Every row records its hit count.

  1  the set's counting pass (k_fs_count + k_fd_scan, HIP events, summed over the batches) next to the SUM of the K
     single-pattern counting passes of find_device on the same patterns (k_fd_count + k_fd_scan), and next to a
     device-to-device copy of the same inflated bytes
  2  find_set_device, a count-only call and then a writing call (positions, ids, lines, counts), host clock,
     synchronised, against K x (count-only + writing find_device), a copy of the K tables to the host and a stable merge
     by position there (np.argsort, kind="stable").  n_hits and d_counts are checked against the K calls in every step,
     for K = 16 positions, ids and lines against the merge
  3  K = 16: select_lines_set_device + read_lines_table_device next to 16 x (select_lines_device +
     read_lines_table_device); reported only

Prints one JSON line; --out FILE writes it too.

    python tools/findset_measure.py [--steps 10] [--warmup 2] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

from find_measure import choose_patterns, stats  # noqa: E402
from gzp_amd import _native, build, synth  # noqa: E402

KS = (1, 4, 16, 64, 256)


def choose_sets(host, which):
    """{name: patterns}: `rare` first, then 12-byte slices of the first 64 MiB at random places, distinct, no newline."""
    head = host[:64 << 20].tobytes()
    rng = np.random.default_rng(20260301)
    slices = [choose_patterns(host)["rare"]]
    while len(slices) < max(KS):
        at = int(rng.integers(0, len(head) - 12))
        cand = head[at:at + 12]
        if b"\n" not in cand and cand not in slices:
            slices.append(cand)
    sets = {"K%d" % k: slices[:k] for k in KS}
    if which == "fastq":
        codes = set()
        while len(codes) < 96:
            codes.add(bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 8)))
        sets["barcodes"] = sorted(codes)
    return sets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bytes", type=int, default=576_716_800)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    n = args.bytes
    res = {"what": "findset_measure", "build_id": build.source_id(), "device": torch.cuda.get_device_name(0), "bytes": n,
           "steps": args.steps, "warmup": args.warmup, "inputs": {}}

    def clock(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, out

    d_in = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    d_copy = torch.empty(n, dtype=torch.uint8, device="cuda:0")
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
        host = d_in.cpu().numpy()
        sets = choose_sets(host, which)
        nl = np.flatnonzero(host == 10)
        one = {"compressed_bytes": int(comp_len), "sets": {}, "shared": {}}
        with _native.DContext(format=_native.FORMAT_BGZF) as d, d.build_index_device(p_comp, comp_len) as ix, \
                d.build_lines_device(ix, p_comp, comp_len) as lt:
            one["members"] = ix.n_members
            d2d = []
            for name, patterns in sets.items():
                K = len(patterns)
                per = [d.find_device(ix, p_comp, comp_len, p) for p in patterns]
                total = sum(per)
                starts = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
                room = max(total, 1)
                d_pos, d_lines = (torch.empty(room, dtype=torch.int64, device="cuda:0") for _ in range(2))
                d_ids = torch.empty(room, dtype=torch.int32, device="cuda:0")
                d_counts = torch.empty(K, dtype=torch.int64, device="cuda:0")
                d_ppos, d_plines = (torch.empty(room, dtype=torch.int64, device="cuda:0") for _ in range(2))
                ids_by_call = np.repeat(np.arange(K), per)
                r = {"set_pass": [], "single_pass_sum": [], "set_write_pass": [], "set_calls": [], "parent_route": [], "inflate": []}
                merged = None

                def parent_route():
                    for k, p in enumerate(patterns):
                        assert d.find_device(ix, p_comp, comp_len, p) == per[k]
                        a = int(starts[k])
                        d.find_device(ix, p_comp, comp_len, p, 10, d_ppos.data_ptr() + 8 * a, d_plines.data_ptr() + 8 * a, max(per[k], 1) if total else 0)
                    pos, lines = d_ppos[:total].cpu().numpy(), d_plines[:total].cpu().numpy()
                    order = np.argsort(pos, kind="stable")
                    return pos[order], ids_by_call[order], lines[order]

                for step in range(args.warmup + args.steps):
                    keep = step >= args.warmup
                    ev0.record()
                    d_copy.copy_(d_in, non_blocking=True)
                    ev1.record()
                    ev1.synchronize()
                    t_c, n_hits = clock(lambda: d.find_set_device(ix, p_comp, comp_len, patterns, d_counts_ptr=d_counts.data_ptr()))
                    set_pass = d.last_find_set_ms()[1]
                    assert n_hits == total and d_counts.cpu().numpy().tolist() == per, (which, name, n_hits, total)
                    t_w, n_hits = clock(lambda: d.find_set_device(ix, p_comp, comp_len, patterns, 10, d_pos.data_ptr(), d_ids.data_ptr(),
                                                                  d_lines.data_ptr(), total, d_counts.data_ptr()))
                    ms = d.last_find_set_ms()
                    assert n_hits == total and d_counts.cpu().numpy().tolist() == per
                    single = 0.0
                    for k, p in enumerate(patterns):
                        assert d.find_device(ix, p_comp, comp_len, p) == per[k]
                        single += d.last_find_ms()[1]
                    t_parent, merged = clock(parent_route)
                    if K == 16:
                        assert np.array_equal(d_pos[:total].cpu().numpy(), merged[0]) and np.array_equal(d_ids[:total].cpu().numpy(), merged[1])
                        assert np.array_equal(d_lines[:total].cpu().numpy(), merged[2])
                        assert np.array_equal(merged[2], np.searchsorted(nl, merged[0], side="left"))
                    if keep:
                        d2d.append(ev0.elapsed_time(ev1))
                        r["set_pass"].append(set_pass)
                        r["single_pass_sum"].append(single)
                        r["set_write_pass"].append(ms[2])
                        r["inflate"].append(ms[0])
                        r["set_calls"].append(t_c + t_w)
                        r["parent_route"].append(t_parent)
                sp, ss = stats(r["set_pass"]), stats(r["single_pass_sum"])
                row = {"K": K, "pattern_bytes": len(patterns[0]), "hits": int(total), "hits_min_max_per_pattern": [int(min(per)), int(max(per))],
                       "run1": {"set_counting_pass_ms": sp, "sum_of_K_single_counting_passes_ms": ss,
                                "factor_median": round(ss["median"] / sp["median"], 2) if sp["median"] > 0 else 0.0,
                                "set_GB_per_s": round(n / (sp["median"] / 1e3) / 1e9, 1) if sp["median"] > 0 else 0.0,
                                "set_max_lt_single_sum_min": bool(sp["max"] < ss["min"])},
                       "run2": {"set_count_plus_write_calls_ms": stats(r["set_calls"]), "parent_route_ms": stats(r["parent_route"]),
                                "set_inflate_kernels_ms": stats(r["inflate"]), "set_writing_pass_ms": stats(r["set_write_pass"]),
                                "set_max_lt_parent_min": bool(max(r["set_calls"]) < min(r["parent_route"]))}}
                if K == 16:  # run 3: the selection and the read of its table
                    L = lt.n_lines
                    d_runs = torch.empty((L // 2 + 1, 2), dtype=torch.int64, device="cuda:0")
                    d_out = torch.empty(n + 64, dtype=torch.uint8, device="cuda:0")
                    t_set, t_single = [], []

                    def select_read(call, pats):
                        runs, _, _ = call(ix, lt, p_comp, comp_len, pats, 1, False, d_runs.data_ptr(), d_runs.shape[0])
                        return d.read_lines_table_device(ix, lt, p_comp, comp_len, d_runs.data_ptr(), runs, d_out.data_ptr(), n + 64)

                    for step in range(args.warmup + args.steps):
                        t, out_len = clock(lambda: select_read(d.select_lines_set_device, patterns))
                        t1 = sum(clock(lambda: select_read(d.select_lines_device, p))[0] for p in patterns)
                        if step >= args.warmup:
                            t_set.append(t)
                            t_single.append(t1)
                    row["run3"] = {"select_set_plus_read_ms": stats(t_set), "K_single_select_plus_read_ms": stats(t_single),
                                   "selected_bytes": int(out_len)}
                    del d_runs, d_out
                one["sets"][name] = row
                print(which, name, json.dumps(row["run1"]), file=sys.stderr, flush=True)
                del d_pos, d_lines, d_ids, d_counts, d_ppos, d_plines
            one["shared"]["d2d_copy_same_bytes_ms"] = stats(d2d)
        res["inputs"][which] = one
        del d_comp, host, nl
    res["conditions"] = {
        "run1_every_K_ge_4": all(row["run1"]["set_max_lt_single_sum_min"] for one in res["inputs"].values()
                                 for row in one["sets"].values() if row["K"] >= 4),
        "run2_every_K_ge_2": all(row["run2"]["set_max_lt_parent_min"] for one in res["inputs"].values()
                                 for row in one["sets"].values() if row["K"] >= 2)}
    res["note"] = ("set_calls, parent_route, run3: host clock around work that is synchronised at both ends; counting passes, writing "
                   "pass, inflate_kernels and d2d: HIP events, summed over the batches.  parent_route = K x (count-only + writing "
                   "find_device) + the K tables to the host + a stable argsort of the positions.  GB/s count the inflated bytes once.")
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
