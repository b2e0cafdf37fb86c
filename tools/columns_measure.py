"""Numeric columns of lines on the MI355X: gzpx_read_columns_table_device against gzpx_read_fields_table_device of the same
field list -- the yardstick: the same walk plus a byte scatter -- and, once, against the path a user had before it: the
fields to the host and numpy's text reader there.  fields_measure.py's two TSVs of about 600 MB (12 and 2,000 decimal
columns a row, 2..8 bytes a field), each compressed at level 1 on the device as BGZF and resident in HBM.  Column lists:
{0} and {0, 3, 11} on both, {1501} on the wide one; each as INT64 and as FLOAT64, values and status bytes both written.
All lines as one range, the range table in device memory.  One process, warm, median / min / max of the steps.

Per column list and type: the HIP-event times of the two stages (last_columns_ms: carries + row scan, the parse), the
inflate in front of them, the host clock around the whole call, synchronised at both ends, the cells that are not OK,
and the parse of a call that is given neither array (it counts and stores no cell).  Per column list: read_fields_table_device's three passes (last_fields_ms) and its whole call, alternating with the
columns calls, and the parse over the fields' writing pass.  On the 12-column file, {0, 3, 11} as INT64: the host path,
timed once, and its array compared with the device's cells.

Prints one JSON line; --out FILE writes it too.

    python tools/columns_measure.py [--steps 5] [--warmup 1] [--out FILE]
"""
import argparse
import io
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from fields_measure import TAB, tsv  # noqa: E402
from find_measure import stats  # noqa: E402
from gzp_amd import _native, build  # noqa: E402

TYPES = (("INT64", _native.COL_INT64), ("FLOAT64", _native.COL_FLOAT64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--bytes", type=int, default=576_716_800)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    res = {"what": "columns_measure", "build_id": build.source_id(), "device": torch.cuda.get_device_name(0), "steps": args.steps,
           "warmup": args.warmup, "inputs": {}}

    def clock(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    inputs = (("tsv 12 columns", 12, {"{0}": [0], "{0, 3, 11}": [0, 3, 11]}),
              ("tsv 2000 columns", 2000, {"{0}": [0], "{0, 3, 11}": [0, 3, 11], "{1501}": [1501]}))
    for which, columns, cases in inputs:
        d_in = torch.from_numpy(tsv(args.bytes, columns, 20260112)).cuda()
        n = d_in.numel()
        torch.cuda.synchronize()
        with _native.Context(format=_native.FORMAT_BGZF, level=1, buffer_size=65280, max_slab_bytes=n) as c:
            cap = c.slab_bound(n)
            d_comp = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
            comp_len, _ = c.compress_slab_device(d_in.data_ptr(), n, d_comp.data_ptr(), cap, True)
        del d_in
        p_comp = d_comp.data_ptr()
        one = {"bytes": int(n), "compressed_bytes": int(comp_len), "field_delim": TAB, "rows": {}}
        with _native.DContext(format=_native.FORMAT_BGZF) as d, d.build_index_device(p_comp, comp_len) as ix, \
                d.build_lines_device(ix, p_comp, comp_len) as lt:
            L = lt.n_lines
            one["members"], one["lines"] = ix.n_members, int(L)
            d_rs = torch.tensor([[0, L]], dtype=torch.int64, device="cuda:0")
            d_cut = torch.empty(n + 64, dtype=torch.uint8, device="cuda:0")
            for name, nums in cases.items():
                fields = [(k, k + 1) for k in nums]
                d_val = torch.empty(len(nums) * L, dtype=torch.int64, device="cuda:0")
                d_st = torch.empty(len(nums) * L, dtype=torch.uint8, device="cuda:0")
                d_bad = torch.empty(len(nums), dtype=torch.int64, device="cuda:0")
                row, t_cut, cut_parts, cut_len = {}, [], {}, 0
                for kind_name, kind in TYPES:
                    print("columns_measure: %s %s %s" % (which, name, kind_name), file=sys.stderr, flush=True)
                    cols = [(k, kind) for k in nums]
                    t_call, parts, got = [], {}, None
                    for step in range(args.warmup + args.steps):
                        box = []
                        a = clock(lambda: box.append(d.read_columns_table_device(ix, lt, p_comp, comp_len, d_rs.data_ptr(), 1, TAB, cols,
                                                                                 d_val.data_ptr(), d_st.data_ptr(), L, d_bad.data_ptr())))
                        cl, search = d.last_columns_ms(), d.last_lines_ms()
                        got = box[0]
                        assert got[0] == L, (which, name, got)
                        b = clock(lambda: box.append(d.read_fields_table_device(ix, lt, p_comp, comp_len, d_rs.data_ptr(), 1, TAB, fields,
                                                                                d_cut.data_ptr(), n)))
                        fl = d.last_fields_ms()
                        cut_len = box[1]
                        box.append(d.read_columns_table_device(ix, lt, p_comp, comp_len, d_rs.data_ptr(), 1, TAB, cols, None, None, 0))
                        bare = d.last_columns_ms()  # (neither array: the same parse, counted, no cell stored)
                        assert box[2][:2] == got[:2], (which, name, box[2])
                        if step >= args.warmup:
                            t_call.append(a)
                            t_cut.append(b)
                            for k, v in (("carries_rows", cl[0]), ("parse", cl[1]), ("two_stages", sum(cl)), ("inflate", search[1]),
                                         ("parse_counts_only", bare[1])):
                                parts.setdefault(k, []).append(v)
                            for k, v in (("carry_scan", fl[0]), ("count_scan", fl[1]), ("write", fl[2]), ("three_passes", sum(fl))):
                                cut_parts.setdefault(k, []).append(v)
                    assert int(d_bad.sum().item()) == got[1] == int((d_st != _native.CELL_OK).sum().item()), (which, name, kind_name)
                    r = {"rows": int(got[0]), "cells_not_ok": int(got[1]), "read_columns_ms": stats(t_call)}
                    r.update({k + "_ms": stats(v) for k, v in parts.items()})
                    row[kind_name] = r
                f = {"out_bytes": int(cut_len), "read_fields_ms": stats(t_cut)}
                f.update({k + "_ms": stats(v) for k, v in cut_parts.items()})
                row["read_fields"] = f
                for kind_name, _ in TYPES:  # (both types' steps alternate with the same fields calls: one write time for both)
                    row[kind_name]["parse_over_fields_write"] = round(row[kind_name]["parse_ms"]["median"] / f["write_ms"]["median"], 3)
                    row[kind_name]["two_stages_over_three_passes"] = round(row[kind_name]["two_stages_ms"]["median"] /
                                                                           f["three_passes_ms"]["median"], 3)
                if columns == 12 and len(nums) == 3:  # the path a user had: cut on the device, the bytes to the host, numpy's reader
                    cols = [(k, _native.COL_INT64) for k in nums]
                    d.read_columns_table_device(ix, lt, p_comp, comp_len, d_rs.data_ptr(), 1, TAB, cols, d_val.data_ptr(), d_st.data_ptr(), L)
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    m = d.read_fields_table_device(ix, lt, p_comp, comp_len, d_rs.data_ptr(), 1, TAB, fields, d_cut.data_ptr(), n)
                    buf = d_cut[:m].cpu().numpy().tobytes()
                    t_copy = time.perf_counter()
                    print("columns_measure: the host path (numpy.loadtxt of %d bytes)" % m, file=sys.stderr, flush=True)
                    host = np.loadtxt(io.BytesIO(buf), dtype=np.int64, delimiter="\t", ndmin=2)
                    t_end = time.perf_counter()
                    assert host.shape == (L, 3) and np.array_equal(host.T, d_val.cpu().numpy().reshape(3, L)), (which, name)
                    row["host_path_ms"] = {"read_fields_and_copy": round((t_copy - t) * 1e3, 1), "numpy_loadtxt": round((t_end - t_copy) * 1e3, 1),
                                           "total": round((t_end - t) * 1e3, 1)}
                    del buf, host
                one["rows"][name] = row
                del d_val, d_st, d_bad
        res["inputs"][which] = one
        del d_comp, d_cut
    res["note"] = ("read_columns, read_fields: host clock around one call each, synchronised at both ends, alternating in one process.  "
                   "carries_rows, parse: HIP events of the two stages (last_columns_ms); inflate: last_lines_ms()[1] of the same call; "
                   "parse_counts_only: the parse stage of a call with d_values and d_status NULL; "
                   "carry_scan, count_scan, write: last_fields_ms of read_fields_table_device for the same field numbers, over both "
                   "types' steps; host_path: read_fields_table_device, the bytes to the host, numpy.loadtxt(dtype=int64), timed once "
                   "and compared with the device's cells.")
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
