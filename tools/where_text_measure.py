"""Selection of lines by the text of their fields on the MI355X: gzpx_where_text_table_device beside its numeric
neighbour and beside the detour it replaces.  Three inputs of about 550 MiB, each compressed at level 1 on the device as
BGZF and resident in HBM: gzpx_synth_fastq_device output (field delimiter ' '), fields_measure.py's TSV of 12 decimal
columns, and a VCF-like TSV of fixed-width rows (CHROM POS ID REF ALT QUAL FILTER INFO; the INFO holds "PASS" too).  All
lines as one range, the range table in device memory, the run table sized (L + 1) / 2.  One process, warm, median / min /
max of the steps.

(a) The parse stage, last_where_ms()[1], of one TEXT term beside the same call with a FLOAT64 (and INT64) term on the same
    field, and of $1 == "chr07" && $6 >= 30 && $7 == "PASS" beside three numeric terms on three fields.
(b) The whole call, host clock, beside the detour: read_fields_device of the three fields, a copy to the host, bytes.split
    and the comparisons in Python (once: it takes seconds); the selected rows of both are compared.
(c) `--numeric-only`: the rows of tools/where_measure.py through where_lines_table_device alone (no user path), so that the
    same file measures another checkout's package: `--tree DIR` imports gzp_amd and the TSV from DIR (the parent commit,
    built there).  `--parent FILE...` and `--branch FILE...` merge such outputs into the result: per row the spread of the
    parent's runs, the median of every branch run, and whether it lies inside.

Prints one JSON line; --out FILE writes it too.

    python tools/where_text_measure.py [--steps 5] [--warmup 1] [--parent FILE... --branch FILE...] [--out FILE]
    python tools/where_text_measure.py --numeric-only [--tree DIR] --out FILE
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if "--tree" in sys.argv[1:-1]:
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from fields_measure import SPACE, TAB, tsv  # noqa: E402
from find_measure import stats  # noqa: E402
from gzp_amd import _native, build  # noqa: E402

INT, FLT = _native.COL_INT64, _native.COL_FLOAT64
LT, EQ, GE = _native.WHERE_LT, _native.WHERE_EQ, _native.WHERE_GE
FILTERS = (b"PASS", b"q10x", b"LowQ", b"SB_f")
VCF_ROW = 64


def vcf(n, seed):
    """About n bytes of rows of 64 bytes: chrNN, POS of 8 digits, rsNNNNNNN, REF, ALT, QUAL dd.d, a FILTER of 4 bytes,
    INFO DP=ddd;AF=0.ddd;FT=ffff with a filter's name of its own."""
    rng = np.random.default_rng(seed)
    rows = n // VCF_ROW
    a = rng.integers(48, 58, (rows, VCF_ROW), dtype=np.uint8)
    a[:, 0:3] = np.frombuffer(b"chr", dtype=np.uint8)
    a[:, 3] = 48 + rng.integers(0, 3, rows)  # chr00 .. chr29
    for at in (5, 14, 24, 26, 28, 33, 38):
        a[:, at] = TAB
    a[:, 15:17] = np.frombuffer(b"rs", dtype=np.uint8)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)
    a[:, 25] = bases[rng.integers(0, 4, rows)]
    a[:, 27] = bases[rng.integers(0, 4, rows)]
    a[:, 31] = ord(".")
    names = np.frombuffer(b"".join(FILTERS), dtype=np.uint8).reshape(4, 4)
    a[:, 34:38] = names[rng.integers(0, 4, rows)]
    a[:, 39:42] = np.frombuffer(b"DP=", dtype=np.uint8)
    a[:, 45:51] = np.frombuffer(b";AF=0.", dtype=np.uint8)
    a[:, 54:58] = np.frombuffer(b";FT=", dtype=np.uint8)
    a[:, 58:62] = names[rng.integers(0, 4, rows)]
    a[:, 62] = ord("x")
    a[:, 63] = 10
    return a.reshape(-1)


def merge(parent_files, branch_files):
    """Row (c): per row and figure the parent's runs, the branch's, and whether each branch run's median lies in the
    parent's spread."""
    parents = [json.load(open(f)) for f in parent_files]
    branches = [json.load(open(f)) for f in branch_files]
    out = {"parent_build_id": parents[0]["build_id"], "branch_build_id": branches[0]["build_id"], "parent_runs": len(parents),
           "branch_runs": len(branches), "rows": {},
           "rule": "spread = [min, max] over a side's runs of every step's value; inside[k] = the median of branch run k lies in the parent's spread"}
    outside = []
    for which, one in branches[0]["inputs"].items():
        for name in one["rows"]:
            r = {}
            for fig in ("where_lines_ms", "parse_predicate_ms", "three_stages_ms"):
                ps = [p["inputs"][which]["rows"][name][fig] for p in parents]
                bs = [b["inputs"][which]["rows"][name][fig] for b in branches]
                lo, hi = min(p["min"] for p in ps), max(p["max"] for p in ps)
                r[fig] = {"parent_medians": [p["median"] for p in ps], "parent_spread": [lo, hi], "branch_medians": [b["median"] for b in bs],
                          "branch_spread": [min(b["min"] for b in bs), max(b["max"] for b in bs)], "inside": [lo <= b["median"] <= hi for b in bs]}
                outside += ["%s / %s / %s / branch run %d: %g outside [%g, %g]" % (which, name, fig, k + 1, b["median"], lo, hi)
                            for k, b in enumerate(bs) if not lo <= b["median"] <= hi]
            out["rows"]["%s / %s" % (which, name)] = r
    out["outside"] = outside
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--bytes", type=int, default=576_716_800)
    ap.add_argument("--numeric-only", action="store_true")
    ap.add_argument("--tree")
    ap.add_argument("--parent", nargs="*", default=[])
    ap.add_argument("--branch", nargs="*", default=[])
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    res = {"what": "where_text_measure" + (", numeric rows" if args.numeric_only else ""), "build_id": build.source_id(),
           "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup, "inputs": {}}

    def clock(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    def resident(which):
        if which == "fastq":
            n = args.bytes
            d_in = torch.empty(n, dtype=torch.uint8, device="cuda:0")
            _native.synth_fastq_device(d_in.data_ptr(), 0, n)
        else:
            host = vcf(args.bytes, 20260113) if which == "vcf-like tsv" else tsv(args.bytes, 12 if "12" in which else 2000, 20260112)
            d_in = torch.from_numpy(host).cuda()
            n = d_in.numel()
        torch.cuda.synchronize()
        with _native.Context(format=_native.FORMAT_BGZF, level=1, buffer_size=65280, max_slab_bytes=n) as c:
            cap = c.slab_bound(n)
            d_comp = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
            comp_len, _ = c.compress_slab_device(d_in.data_ptr(), n, d_comp.data_ptr(), cap, True)
        return d_comp, comp_len, n

    def rows_of(which, fd, cases, call_name):
        d_comp, comp_len, n = resident(which)
        p_comp = d_comp.data_ptr()
        one = {"bytes": int(n), "compressed_bytes": int(comp_len), "field_delim": fd, "rows": {}}
        with _native.DContext(format=_native.FORMAT_BGZF) as d, d.build_index_device(p_comp, comp_len) as ix, \
                d.build_lines_device(ix, p_comp, comp_len) as lt:
            L = lt.n_lines
            one["members"], one["lines"] = ix.n_members, int(L)
            d_rs = torch.tensor([[0, L]], dtype=torch.int64, device="cuda:0")
            runs_cap = (L + 1) // 2
            d_runs = torch.empty(2 * runs_cap, dtype=torch.int64, device="cuda:0")
            call = getattr(d, call_name)
            for name, terms in (cases(d, ix, lt, p_comp, comp_len, d_rs, L) if callable(cases) else cases).items():
                print("where_text_measure: %s %s" % (which, name), file=sys.stderr, flush=True)
                t_call, parts, got = [], {}, None
                for step in range(args.warmup + args.steps):
                    box = []
                    a = clock(lambda: box.append(call(ix, lt, p_comp, comp_len, d_rs.data_ptr(), 1, fd, terms, False, False, d_runs.data_ptr(),
                                                      runs_cap)))
                    wh, search = d.last_where_ms(), d.last_lines_ms()
                    got = box[0]
                    if step >= args.warmup:
                        t_call.append(a)
                        for k, v in (("carries_rows", wh[0]), ("parse_predicate", wh[1]), ("runs", wh[2]), ("three_stages", sum(wh)),
                                     ("inflate", search[1])):
                            parts.setdefault(k, []).append(v)
                assert got[2] == L, (which, name, got)
                r = {"terms": [[t[0], t[1], t[2], t[3].decode("latin-1") if isinstance(t[3], bytes) else t[3]] for t in terms], "runs": int(got[0]),
                     "selected": int(got[1]), "rows": int(got[2]), "cells_not_ok": int(got[3]), "selectivity": round(got[1] / L, 5),
                     "where_lines_ms": stats(t_call)}
                r.update({k + "_ms": stats(v) for k, v in parts.items()})
                one["rows"][name] = r
            if which == "vcf-like tsv" and not args.numeric_only:
                one["detour"] = detour(d, ix, lt, p_comp, comp_len, n, L, one["rows"]["$1 == chr07 && $6 >= 30 && $7 == PASS"])
        res["inputs"][which] = one

    def detour(d, ix, lt, p_comp, comp_len, n, L, row):
        """What a user had: read_fields_device of the three fields, the bytes to the host, split and compare there."""
        d_out = torch.empty(n, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out_len, _ = d.read_fields_device(ix, lt, p_comp, comp_len, [(0, L)], TAB, [(0, 1), (5, 7)], d_out.data_ptr(), n)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        buf = d_out[:out_len].cpu().numpy().tobytes()
        t2 = time.perf_counter()
        selected = 0
        for line in buf.split(b"\n"):
            p = line.split(b"\t")
            if len(p) == 3 and p[0] == b"chr07" and p[2] == b"PASS" and float(p[1]) >= 30.0:
                selected += 1
        t3 = time.perf_counter()
        assert selected == row["selected"], (selected, row["selected"])
        total = (t3 - t0) * 1e3
        return {"fields": [[0, 1], [5, 7]], "out_bytes": int(out_len), "read_fields_ms": round((t1 - t0) * 1e3, 3), "copy_to_host_ms": round((t2 - t1) * 1e3, 3),
                "split_and_compare_ms": round((t3 - t2) * 1e3, 3), "total_ms": round(total, 3), "selected": selected, "steps": 1,
                "detour_over_call": round(total / row["where_lines_ms"]["median"], 1)}

    def numeric_cases(d, ix, lt, p_comp, comp_len, d_rs, L):
        """tools/where_measure.py's term sets: the constants are quantiles of the columns themselves."""
        nums = [0, 3, 11]
        d_val = torch.empty(3 * L, dtype=torch.int64, device="cuda:0")
        d.read_columns_table_device(ix, lt, p_comp, comp_len, d_rs.data_ptr(), 1, TAB, [(k, INT) for k in nums], d_val.data_ptr(), None, L)
        ordered = [torch.sort(d_val[j * L:(j + 1) * L]).values for j in range(3)]
        q = lambda j, s: int(ordered[j][min(max(int(s * L), 0), L - 1)].item())  # noqa: E731
        cases = {}
        for s in (0.001, 0.5, 0.999):
            each = s ** (1.0 / 3.0)
            cases["{0}, %g" % s] = [(0, INT, LT, q(0, s))]
            cases["{0, 3, 11}, %g" % s] = [(k, INT, LT, q(j, each)) for j, k in enumerate(nums)]
            cases["{0} two terms, %g" % s] = [(0, INT, GE, q(0, (1 - s) / 2)), (0, INT, LT, q(0, (1 + s) / 2))]
        return cases

    if args.numeric_only:
        for which in ("tsv 12 columns", "tsv 2000 columns"):
            rows_of(which, TAB, numeric_cases, "where_lines_table_device")
    else:
        TEXT, PREFIX = _native.COL_TEXT, _native.WHERE_PREFIX
        rows_of("fastq", SPACE, {"text PREFIX $1": [(0, TEXT, PREFIX, b"@")], "text EQ $1, 64 bytes": [(0, TEXT, EQ, b"@" + b"A" * 63)],
                                 "float64 LT $1": [(0, FLT, LT, 0.0)]}, "where_text_table_device")
        rows_of("tsv 12 columns", TAB, {"text EQ $1": [(0, TEXT, EQ, b"4498")], "float64 EQ $1": [(0, FLT, EQ, 4498.0)], "int64 EQ $1": [(0, INT, EQ, 4498)],
                                        "text LT $1, $4, $12": [(k, TEXT, LT, b"5") for k in (0, 3, 11)],
                                        "float64 LT $1, $4, $12": [(k, FLT, LT, 5e5) for k in (0, 3, 11)]}, "where_text_table_device")
        rows_of("vcf-like tsv", TAB, {"text EQ $6": [(5, TEXT, EQ, b"30.0")], "float64 EQ $6": [(5, FLT, EQ, 30.0)], "text EQ $1": [(0, TEXT, EQ, b"chr07")],
                                      "text EQ $8, 24 bytes": [(7, TEXT, EQ, b"DP=500;AF=0.500;FT=PASSx")],
                                      "$1 == chr07 && $6 >= 30 && $7 == PASS": [(0, TEXT, EQ, b"chr07"), (5, FLT, GE, 30.0), (6, TEXT, EQ, b"PASS")],
                                      "$2 < 5e7 && $6 >= 30 && $8 not OK (numeric on three fields)": [(1, INT, LT, 50_000_000), (5, FLT, GE, 30.0),
                                                                                                     (7, FLT, _native.WHERE_NOT_OK, 0)]},
                "where_text_table_device")
        if args.parent and args.branch:
            res["existing_entry_points"] = merge(args.parent, args.branch)
    res["note"] = ("where_lines: host clock around one call, synchronised at both ends.  carries_rows, parse_predicate, runs: HIP events of the "
                   "three stages (last_where_ms); inflate: last_lines_ms()[1] of the same call.  detour: read_fields_device of the three fields, "
                   "the bytes to the host, bytes.split and the comparisons in Python, once.  existing_entry_points: where_lines_table_device "
                   "with where_measure.py's rows, measured by this file's --numeric-only in processes of their own: the parent commit's package "
                   "and this build's several times each.")
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
