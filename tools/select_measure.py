"""Selection of lines by content on the MI355X: gzpx_select_lines_device + gzpx_read_lines_table_device against the same
result through the entry points that were there before them.  Two inputs, each compressed at level 1 on the device as
BGZF and resident in HBM: bench.py's 550 MiB text slab (records of one line) and 550 MiB of gzpx_synth_fastq_device
output (records of one line and of four).  One process, warm, median / min / max of the steps.  Three patterns per
input, chosen from the input itself as tools/find_measure.py does: a 12-byte slice with on the order of 1,000 hits
(`rare`), the same with its last byte replaced so that it never matches (`absent`), and "\\n", which every record holds
(`every`); each plain and inverted.  The inverted `rare` row is the dense case: nearly all records, a second inflate of
nearly everything and about as many boundary walks as there are runs.

  new path   one select_lines_device with a table of ceil(R / 2) entries, then one read_lines_table_device on it
  yardstick  count-only find_device; writing find_device with d_lines; the line numbers to the host; numpy unique,
             division by the group, runs; read_lines_device

Both host clock, synchronised at both ends.  The two paths' bytes are compared on the device once per row.  Per row also
the HIP-event times of the new path's kernels: select's inflate, its count + scan + mark pass (and, beside it, find's count
+ scan pass of the same pattern: the difference is k_sl_mark), the runs kernels, and the read's four stages, of which the
third is k_ln_find.

Prints one JSON line; --out FILE writes it too.

    python tools/select_measure.py [--steps 10] [--warmup 2] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from find_measure import choose_patterns, stats  # noqa: E402
from gzp_amd import _native, build, synth  # noqa: E402


def host_runs(lines, g, L, invert):
    """The runs of the selected records as line ranges, from the line numbers of the hits."""
    R = -(-L // g)
    sel = np.zeros(R, dtype=bool)
    sel[np.unique(lines // g)] = True
    if invert:
        sel = ~sel
    edge = np.diff(np.concatenate([[0], sel.astype(np.int8), [0]]))
    return np.stack([g * np.flatnonzero(edge == 1), np.minimum(g * np.flatnonzero(edge == -1), L)], axis=1).astype(np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bytes", type=int, default=576_716_800)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    n = args.bytes
    res = {"what": "select_measure", "build_id": build.source_id(), "device": torch.cuda.get_device_name(0), "bytes": n,
           "steps": args.steps, "warmup": args.warmup, "inputs": {}}

    def clock(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    d_in = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    d_new = torch.empty(n + 64, dtype=torch.uint8, device="cuda:0")
    d_old = torch.empty(n + 64, dtype=torch.uint8, device="cuda:0")
    for which, groups in (("text_slab", (1,)), ("fastq", (1, 4))):
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
        chosen = choose_patterns(d_in.cpu().numpy())
        patterns = {"rare": chosen["rare"], "absent": chosen["absent"], "every": b"\n"}
        one = {"compressed_bytes": int(comp_len), "patterns": {k: v.hex() for k, v in patterns.items()}, "rows": {}}
        with _native.DContext(format=_native.FORMAT_BGZF) as d, d.build_index_device(p_comp, comp_len) as ix, \
                d.build_lines_device(ix, p_comp, comp_len) as lt:
            L = lt.n_lines
            one["members"], one["lines"] = ix.n_members, int(L)
            d_lines = torch.empty(max(L, 1), dtype=torch.int64, device="cuda:0")
            d_runs = torch.empty((-(-L // 2) + 1, 2), dtype=torch.int64, device="cuda:0")
            for g in groups:
                cap_runs = -(-(-(-L // g)) // 2)
                for name, pat in patterns.items():
                    for invert in (False, True):
                        row = "%s g=%d%s" % (name, g, " inverted" if invert else "")
                        print("select_measure: %s %s" % (which, row), file=sys.stderr, flush=True)
                        t_new, t_old, parts, counts = [], [], {}, None

                        def new_path():
                            runs, records, hits = d.select_lines_device(ix, lt, p_comp, comp_len, pat, g, invert, d_runs.data_ptr(), cap_runs)
                            sel = d.last_select_ms()
                            out = d.read_lines_table_device(ix, lt, p_comp, comp_len, d_runs.data_ptr(), runs, d_new.data_ptr(), n)
                            return (runs, records, hits, out), sel, d.last_lines_ms()

                        def yardstick():
                            hits = d.find_device(ix, p_comp, comp_len, pat)
                            count_pass = d.last_find_ms()[1]
                            d.find_device(ix, p_comp, comp_len, pat, 10, None, d_lines.data_ptr(), hits)
                            lines = d_lines[:hits].cpu().numpy()
                            runs = host_runs(lines, g, L, invert)
                            out = d.read_lines_device(ix, lt, p_comp, comp_len, runs, d_old.data_ptr(), n)[0] if runs.size else 0
                            return (runs.shape[0], out), count_pass

                        for step in range(args.warmup + args.steps):
                            got_new, got_old = [], []
                            a = clock(lambda: got_new.append(new_path()))
                            b = clock(lambda: got_old.append(yardstick()))
                            (runs, records, hits, out), sel, rd = got_new[0]
                            (old_runs, old_out), count_pass = got_old[0]
                            assert (runs, out) == (old_runs, old_out), (which, row, runs, out, old_runs, old_out)
                            if step == 0:
                                assert torch.equal(d_new[:out], d_old[:out]), (which, row)
                            if step >= args.warmup:
                                t_new.append(a)
                                t_old.append(b)
                                for k, v in (("select_inflate", sel[0]), ("select_count_scan_mark", sel[1]), ("select_runs", sel[2]),
                                             ("find_count_scan", count_pass), ("read_tiles_select", rd[0]), ("read_inflate", rd[1]),
                                             ("read_k_ln_find", rd[2]), ("read_gather", rd[3])):
                                    parts.setdefault(k, []).append(v)
                            counts = {"runs": int(runs), "records": int(records), "hits": int(hits), "bytes_read": int(out)}
                        new, old = stats(t_new), stats(t_old)
                        kernels = {k + "_ms": stats(v) for k, v in parts.items()}
                        mark = float(np.median(parts["select_count_scan_mark"]) - np.median(parts["find_count_scan"]))
                        kernels["k_sl_mark_ms_by_difference"] = round(mark, 4)
                        for k in ("select_runs", "read_k_ln_find"):
                            kernels[k + "_share_of_new_path"] = round(float(np.median(parts[k])) / new["median"], 4)
                        kernels["k_sl_mark_share_of_new_path"] = round(mark / new["median"], 4)
                        one["rows"][row] = dict(counts, new_path_ms=new, yardstick_ms=old, new_max_lt_yardstick_min=bool(new["max"] < old["min"]),
                                                kernels=kernels)
        res["inputs"][which] = one
        del d_comp, d_lines, d_runs
    res["note"] = ("new_path, yardstick: host clock around work that is synchronised at both ends, alternating in one process.  "
                   "kernels: HIP events of the new path's two calls (select's first two summed over its batches); find_count_scan is "
                   "the yardstick's count-only find of the same step.")
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
