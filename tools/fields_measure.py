"""Fields of lines on the MI355X: gzpx_read_fields_table_device against the read by line of the same ranges, whose
gather moves the same input bytes, and against the path a user had before it: that read, a copy to the host, and
bytes.split / join there.  Three inputs of about 550 MiB, each compressed at level 1 on the device as BGZF and resident in
HBM: gzpx_synth_fastq_device output (field delimiter ' '), a TSV of 12 decimal columns a row and a TSV of 2,000 columns
a row, both made here with numpy.  Three field lists per input: -f1-8, one late column, and everything (S = [0, inf),
which must reproduce the read by line byte for byte -- compared on the device once per row).  All lines as one range,
the range table in device memory.  One process, warm, median / min / max of the steps.

Per row: the HIP-event times of the three passes (last_fields_ms), their sum, the gather of read_lines_table_device
(last_lines_ms()[3]) and the ratio of the two; the host clock around both calls, synchronised at both ends; and for
-f1-8 the host path, timed once.

Prints one JSON line; --out FILE writes it too.

    python tools/fields_measure.py [--steps 5] [--warmup 1] [--out FILE]
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

from find_measure import stats  # noqa: E402
from gzp_amd import _native, build  # noqa: E402

TAB, NL, SPACE = 9, 10, 32
END = _native.FIELDS_TO_END


def tsv(n, columns, seed, chunk=32 << 20):
    """About n bytes of rows of `columns` decimal fields of 1..7 digits: random digits, a tab or a newline behind every
    field."""
    rng = np.random.default_rng(seed)
    parts, size = [], 0
    while size < n:
        widths = rng.integers(2, 9, chunk // 5)
        ends = np.cumsum(widths) - 1
        ends = ends[:ends.size // columns * columns]
        a = rng.integers(48, 58, int(ends[-1]) + 1, dtype=np.uint8)
        a[ends] = TAB
        a[ends[columns - 1::columns]] = NL
        parts.append(a)
        size += a.size
    return np.concatenate(parts)


def host_cut(buf, fd, fields):
    """cut on the host, as a user writes it: split every line, keep the listed fields, join."""
    f = bytes([fd])
    keep = [k for b, e in fields for k in range(b, e)]
    def cut(line):
        cols = line.split(f)
        return f.join(cols[k] for k in keep if k < len(cols))

    lines = buf.split(b"\n")
    tail = lines.pop()  # what stands behind the last newline: an unterminated line, or nothing
    return b"".join(cut(line) + b"\n" for line in lines) + (cut(tail) if tail else b"")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--bytes", type=int, default=576_716_800)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    res = {"what": "fields_measure", "build_id": build.source_id(), "device": torch.cuda.get_device_name(0), "steps": args.steps,
           "warmup": args.warmup, "inputs": {}}

    def clock(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    inputs = (("fastq", SPACE, {"f1-8": [(0, 8)], "late column (2)": [(1, 2)], "everything": [(0, END)]}),
              ("tsv 12 columns", TAB, {"f1-8": [(0, 8)], "late column (11)": [(10, 11)], "everything": [(0, END)]}),
              ("tsv 2000 columns", TAB, {"f1-8": [(0, 8)], "late column (1501)": [(1500, 1501)], "everything": [(0, END)]}))
    for which, fd, cases in inputs:
        if which == "fastq":
            n = args.bytes
            d_in = torch.empty(n, dtype=torch.uint8, device="cuda:0")
            _native.synth_fastq_device(d_in.data_ptr(), 0, n)
        else:
            d_in = torch.from_numpy(tsv(args.bytes, 12 if "12" in which else 2000, 20260112)).cuda()
            n = d_in.numel()
        torch.cuda.synchronize()
        with _native.Context(format=_native.FORMAT_BGZF, level=1, buffer_size=65280, max_slab_bytes=n) as c:
            cap = c.slab_bound(n)
            d_comp = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
            comp_len, _ = c.compress_slab_device(d_in.data_ptr(), n, d_comp.data_ptr(), cap, True)
        del d_in
        p_comp = d_comp.data_ptr()
        d_new = torch.empty(n + 64, dtype=torch.uint8, device="cuda:0")
        d_old = torch.empty(n + 64, dtype=torch.uint8, device="cuda:0")
        one = {"bytes": int(n), "compressed_bytes": int(comp_len), "field_delim": fd, "rows": {}}
        with _native.DContext(format=_native.FORMAT_BGZF) as d, d.build_index_device(p_comp, comp_len) as ix, \
                d.build_lines_device(ix, p_comp, comp_len) as lt:
            L = lt.n_lines
            one["members"], one["lines"] = ix.n_members, int(L)
            d_rs = torch.tensor([[0, L]], dtype=torch.int64, device="cuda:0")
            for name, fields in cases.items():
                print("fields_measure: %s %s" % (which, name), file=sys.stderr, flush=True)
                t_new, t_old, parts = [], [], {}
                for step in range(args.warmup + args.steps):
                    got = []
                    a = clock(lambda: got.append(d.read_fields_table_device(ix, lt, p_comp, comp_len, d_rs.data_ptr(), 1, fd, fields,
                                                                            d_new.data_ptr(), n)))
                    fl, search = d.last_fields_ms(), d.last_lines_ms()
                    b = clock(lambda: got.append(d.read_lines_table_device(ix, lt, p_comp, comp_len, d_rs.data_ptr(), 1, d_old.data_ptr(), n)))
                    rd = d.last_lines_ms()
                    assert got[1] == n
                    if step == 0 and name == "everything":
                        assert got[0] == n and torch.equal(d_new[:n], d_old[:n]), (which, name)
                    if step >= args.warmup:
                        t_new.append(a)
                        t_old.append(b)
                        for k, v in (("carry_scan", fl[0]), ("count_scan", fl[1]), ("write", fl[2]), ("three_passes", sum(fl)),
                                     ("fields_inflate", search[1]), ("read_lines_inflate", rd[1]), ("read_lines_gather", rd[3])):
                            parts.setdefault(k, []).append(v)
                row = {"out_bytes": int(got[0]), "read_fields_ms": stats(t_new), "read_lines_ms": stats(t_old)}
                row.update({k + "_ms": stats(v) for k, v in parts.items()})
                row["three_passes_over_gather"] = round(float(np.median(parts["three_passes"]) / np.median(parts["read_lines_gather"])), 3)
                if name == "f1-8":  # the path a user had: the lines to the host, split and join there (once: it takes seconds)
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    d.read_lines_table_device(ix, lt, p_comp, comp_len, d_rs.data_ptr(), 1, d_old.data_ptr(), n)
                    buf = d_old[:n].cpu().numpy().tobytes()
                    t_copy = time.perf_counter()
                    cut = host_cut(buf, fd, fields)
                    t_end = time.perf_counter()
                    assert cut == d_new[:got[0]].cpu().numpy().tobytes(), (which, name)
                    row["host_path_ms"] = {"read_and_copy": round((t_copy - t) * 1e3, 1), "split_join": round((t_end - t_copy) * 1e3, 1),
                                           "total": round((t_end - t) * 1e3, 1)}
                    del buf, cut
                one["rows"][name] = row
        res["inputs"][which] = one
        del d_comp, d_new, d_old
    res["note"] = ("read_fields, read_lines: host clock around one call each, synchronised at both ends, alternating in one process.  "
                   "carry_scan, count_scan, write: HIP events of the three passes (last_fields_ms); read_lines_gather: last_lines_ms()[3] "
                   "of the read by line of the same range; host_path: timed once.")
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
