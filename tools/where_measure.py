"""Selection of lines by their numbers on the MI355X: gzpx_where_lines_table_device against the three things it stands
beside -- the parse of gzpx_read_columns_table_device for the same columns with no arrays given (DESIGN.md §8l's "no
stores"), the runs pass of gzpx_select_lines_device over as many lines, and the path a user had before it: the cells of
read_columns_table_device into arrays, the predicate and the runs in torch on the device.  fields_measure.py's two TSVs
of about 600 MB (12 and 2,000 decimal columns a row), each compressed at level 1 on the device as BGZF and resident in
HBM.  Terms on {0}, on {0, 3, 11} (one `<` a column, all must hold) and two terms on column 0 (lo <= c0 < hi); the
constants are quantiles of the columns themselves, read on the device, for selectivities of about 0.1 %, 50 % and 99.9 %.
All lines as one range, the range table in device memory, the run table sized (L + 1) / 2.  One process, warm, median /
min / max of the steps.

Per term set and selectivity: the HIP-event times of the three stages (last_where_ms), the host clock around the whole
call, synchronised at both ends, the runs and the selected rows; the no-stores parse of read_columns for the same
columns; the user's path, whose run table is compared with the call's, entry by entry.  Per input:
select_lines_device's [2] for one pattern.

Prints one JSON line; --out FILE writes it too.

    python tools/where_measure.py [--steps 5] [--warmup 1] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from fields_measure import TAB, tsv  # noqa: E402
from find_measure import stats  # noqa: E402
from gzp_amd import _native, build  # noqa: E402

INT = _native.COL_INT64
SELECTIVITIES = (0.001, 0.5, 0.999)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--bytes", type=int, default=576_716_800)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    res = {"what": "where_measure", "build_id": build.source_id(), "device": torch.cuda.get_device_name(0), "steps": args.steps,
           "warmup": args.warmup, "inputs": {}}

    def clock(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    for which, columns in (("tsv 12 columns", 12), ("tsv 2000 columns", 2000)):
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
            runs_cap = (L + 1) // 2
            d_runs = torch.empty(2 * runs_cap, dtype=torch.int64, device="cuda:0")
            d_val = torch.empty(3 * L, dtype=torch.int64, device="cuda:0")
            d_st = torch.empty(3 * L, dtype=torch.uint8, device="cuda:0")
            nums = [0, 3, 11]
            cols3 = [(k, INT) for k in nums]
            d.read_columns_table_device(ix, lt, p_comp, comp_len, d_rs.data_ptr(), 1, TAB, cols3, d_val.data_ptr(), d_st.data_ptr(), L)
            ordered = [torch.sort(d_val[j * L:(j + 1) * L]).values for j in range(3)]

            def quantile(j, q):
                return int(ordered[j][min(max(int(q * L), 0), L - 1)].item())

            # the runs pass of select_lines_device over the same lines
            t_sel, sel_got = [], None
            for step in range(args.warmup + args.steps):
                sel_got = d.select_lines_device(ix, lt, p_comp, comp_len, b"\t5", 1, False, d_runs.data_ptr(), runs_cap)
                if step >= args.warmup:
                    t_sel.append(d.last_select_ms()[2])
            one["select_lines"] = {"pattern": "\\t5", "runs": int(sel_got[0]), "records": int(sel_got[1]), "runs_pass_ms": stats(t_sel)}

            for s in SELECTIVITIES:
                each = s ** (1.0 / 3.0)
                cases = {"{0}": [(0, INT, _native.WHERE_LT, quantile(0, s))],
                         "{0, 3, 11}": [(k, INT, _native.WHERE_LT, quantile(j, each)) for j, k in enumerate(nums)],
                         "{0} two terms": [(0, INT, _native.WHERE_GE, quantile(0, (1 - s) / 2)), (0, INT, _native.WHERE_LT, quantile(0, (1 + s) / 2))]}
                for name, terms in cases.items():
                    print("where_measure: %s %s %g" % (which, name, s), file=sys.stderr, flush=True)
                    cols = [(k, INT) for k in sorted({t[0] for t in terms})]
                    t_call, t_user, parts, got, user_runs = [], [], {}, None, None

                    def user():
                        # the path a user had: the cells into arrays, the predicate and the runs in torch, the table on the device
                        d.read_columns_table_device(ix, lt, p_comp, comp_len, d_rs.data_ptr(), 1, TAB, cols, d_val.data_ptr(), d_st.data_ptr(), L)
                        col = {k: j for j, (k, _) in enumerate(cols)}
                        ok = torch.ones(L, dtype=torch.bool, device="cuda:0")
                        for k, _, op, v in terms:
                            x = d_val[col[k] * L:(col[k] + 1) * L]
                            ok &= (d_st[col[k] * L:(col[k] + 1) * L] == 0) & ((x < v) if op == _native.WHERE_LT else (x >= v))
                        pad = torch.zeros(L + 2, dtype=torch.int8, device="cuda:0")
                        pad[1:L + 1] = ok
                        edge = pad[1:] - pad[:-1]
                        return torch.stack([torch.nonzero(edge == 1).flatten(), torch.nonzero(edge == -1).flatten()], dim=1).contiguous()

                    for step in range(args.warmup + args.steps):
                        box = []
                        a = clock(lambda: box.append(d.where_lines_table_device(ix, lt, p_comp, comp_len, d_rs.data_ptr(), 1, TAB, terms, False,
                                                                                False, d_runs.data_ptr(), runs_cap)))
                        wh, search = d.last_where_ms(), d.last_lines_ms()
                        got = box[0]
                        d.read_columns_table_device(ix, lt, p_comp, comp_len, d_rs.data_ptr(), 1, TAB, cols, None, None, 0)
                        bare = d.last_columns_ms()  # (neither array: the same parse, counted, no cell stored)
                        b = clock(lambda: box.append(user()))
                        user_runs = box[1]
                        if step >= args.warmup:
                            t_call.append(a)
                            t_user.append(b)
                            for k, v in (("carries_rows", wh[0]), ("parse_predicate", wh[1]), ("runs", wh[2]), ("three_stages", sum(wh)),
                                         ("inflate", search[1]), ("columns_parse_no_stores", bare[1])):
                                parts.setdefault(k, []).append(v)
                    assert got[2] == L and got[0] == user_runs.shape[0], (which, name, s, got, user_runs.shape)
                    assert torch.equal(d_runs[:2 * got[0]].view(-1, 2), user_runs), (which, name, s, "the run tables differ")
                    r = {"terms": [list(t) for t in terms], "runs": int(got[0]), "selected": int(got[1]), "rows": int(got[2]),
                         "cells_not_ok": int(got[3]), "selectivity": round(got[1] / L, 5), "where_lines_ms": stats(t_call),
                         "user_path_ms": stats(t_user)}
                    r.update({k + "_ms": stats(v) for k, v in parts.items()})
                    r["parse_over_no_stores"] = round(r["parse_predicate_ms"]["median"] / r["columns_parse_no_stores_ms"]["median"], 3)
                    r["runs_over_select_runs"] = round(r["runs_ms"]["median"] / one["select_lines"]["runs_pass_ms"]["median"], 3)
                    r["user_path_over_call"] = round(r["user_path_ms"]["median"] / r["where_lines_ms"]["median"], 3)
                    one["rows"]["%s, %g" % (name, s)] = r
            del ordered, d_val, d_st, d_runs
        res["inputs"][which] = one
        del d_comp
    res["note"] = ("where_lines, user_path: host clock around one call / one pass of the user's path, synchronised at both ends, alternating "
                   "in one process.  carries_rows, parse_predicate, runs: HIP events of the three stages (last_where_ms); inflate: "
                   "last_lines_ms()[1] of the same call; columns_parse_no_stores: last_columns_ms()[1] of read_columns_table_device for "
                   "the same columns with d_values and d_status NULL; select_lines.runs_pass: last_select_ms()[2]; user_path: "
                   "read_columns_table_device with both arrays, the predicate and the edges in torch on the device, the run table "
                   "left in device memory and compared with the call's.")
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
