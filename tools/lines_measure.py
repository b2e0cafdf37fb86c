"""Reads by line on the MI355X: the line table and gzpx_read_lines_device against what they replace and what they ride
on.  Two inputs, each compressed at level 1 on the device as BGZF and resident in HBM: bench.py's 550 MiB text slab, and
550 MiB of gzpx_synth_fastq_device output; delimiter '\\n'.  One process, warm, median / min / max of the steps.

  1  k_ln_count alone (HIP events, summed over the batches of a build) next to a device-to-device copy of the same
     inflated bytes (the copy moves twice the bytes of the read-only pass)
  2  build_lines_device (host clock, synchronised) against the one-time cost of the detour: decompress_stream_device of
     everything + a copy to the host + np.flatnonzero(buf == 10); and next to plain decompress_stream_device
  3  read_lines_device for (i) 10,000 random ranges of 4 lines, (ii) 1,000 ranges of 10,000 lines, (iii) all lines, each
     next to read_ranges_device on the equivalent byte ranges (computed beforehand): the four stages, and the ratio

Prints one JSON line; --out FILE writes it too.

    python tools/lines_measure.py [--steps 10] [--warmup 2] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bytes", type=int, default=576_716_800)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    n = args.bytes
    res = {"what": "lines_measure", "build_id": build.source_id(), "device": torch.cuda.get_device_name(0), "bytes": n,
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
        one = {"compressed_bytes": int(comp_len)}
        with _native.DContext(format=_native.FORMAT_BGZF) as d, d.build_index_device(p_comp, comp_len) as ix:
            one["members"] = ix.n_members
            found = {}

            def new_build():
                d.build_lines_device(ix, p_comp, comp_len).close()

            def detour():
                d.decompress_stream_device(p_comp, comp_len, d_full.data_ptr(), n + 64)
                h_full.copy_(d_full[:n])
                found["pos"] = np.flatnonzero(h_full.numpy() == 10)

            def plain():
                d.decompress_stream_device(p_comp, comp_len, d_full.data_ptr(), n + 64)

            rows = {"build": [], "detour": [], "plain": [], "count": [], "build_inflate": [], "d2d": []}
            for step in range(args.warmup + args.steps):
                t_b = clock(new_build)
                inflate_ms, count_ms = d.last_lines_build_ms()
                t_d, t_p = clock(detour), clock(plain)
                ev0.record()
                d_copy[:n].copy_(d_full[:n], non_blocking=True)
                ev1.record()
                ev1.synchronize()
                if step >= args.warmup:
                    rows["build"].append(t_b)
                    rows["detour"].append(t_d)
                    rows["plain"].append(t_p)
                    rows["count"].append(count_ms)
                    rows["build_inflate"].append(inflate_ms)
                    rows["d2d"].append(ev0.elapsed_time(ev1))
            cnt, d2d = stats(rows["count"]), stats(rows["d2d"])
            one["run1"] = {"k_ln_count_ms": cnt, "d2d_copy_same_bytes_ms": d2d,
                           "count_GB_per_s": round(n / (cnt["median"] / 1e3) / 1e9, 1) if cnt["median"] > 0 else 0.0,
                           "d2d_GB_per_s": round(n / (d2d["median"] / 1e3) / 1e9, 1) if d2d["median"] > 0 else 0.0,
                           "count_not_slower_than_copy": bool(cnt["median"] <= d2d["median"])}
            one["run2"] = {"build_lines_ms": stats(rows["build"]), "build_inflate_kernels_ms": stats(rows["build_inflate"]),
                           "detour_inflate_copy_flatnonzero_ms": stats(rows["detour"]),
                           "plain_stream_device_ms": stats(rows["plain"]),
                           "build_max_lt_detour_min": bool(max(rows["build"]) < min(rows["detour"]))}
            # the yardstick of the checks below and the source of the equivalent byte ranges: the detour's own result
            pos = found["pos"].astype(np.int64)
            D = int(pos.size)
            L = D if int(h_full[n - 1]) == 10 else D + 1
            start = np.concatenate([[0], pos + 1, [n] if L > D else []]).astype(np.int64)
            rng = np.random.default_rng(20260105)
            sets = {}
            a = rng.integers(0, L - 4 + 1, 10000)
            sets["i_10000x4_lines"] = np.stack([a, a + 4], axis=1)
            a = rng.integers(0, L - 10000 + 1, 1000)
            sets["ii_1000x10000_lines"] = np.stack([a, a + 10000], axis=1)
            sets["iii_all_lines"] = np.array([[0, L]])
            with d.build_lines_device(ix, p_comp, comp_len) as lt:
                assert (lt.n_delims, lt.n_lines) == (D, L)
                one["lines"], one["tiles"] = L, int(lt.prefix().size - 1)
                one["run3"] = {}
                for name, lr in sets.items():
                    lr = lr.astype(np.uint64)
                    br = np.stack([start[lr[:, 0].astype(np.int64)], start[lr[:, 1].astype(np.int64)]], axis=1).astype(np.uint64)
                    total = int((br[:, 1] - br[:, 0]).sum())
                    d_out = torch.empty(total + 64, dtype=torch.uint8, device="cuda:0")

                    def by_line():
                        got, _, _ = d.read_lines_device(ix, lt, p_comp, comp_len, lr, d_out.data_ptr(), total)
                        assert got == total

                    def by_byte():
                        got, _ = d.read_ranges_device(ix, p_comp, comp_len, br, d_out.data_ptr(), total)
                        assert got == total

                    r3 = {"line": [], "byte": [], "stages": [], "byte_stages": []}
                    for step in range(args.warmup + args.steps):
                        t_l = clock(by_line)
                        st, members = d.last_lines_ms(), d.last_lines_members()
                        t_r = clock(by_byte)
                        if step >= args.warmup:
                            r3["line"].append(t_l)
                            r3["byte"].append(t_r)
                            r3["stages"].append(st)
                            r3["byte_stages"].append(d.last_ranges_ms())
                    # the call's answer against the slab, once, behind the timers
                    got, offs, got_br = d.read_lines_device(ix, lt, p_comp, comp_len, lr, d_out.data_ptr(), total)
                    assert np.array_equal(got_br, br)
                    k = int(np.argmax(br[:, 1] - br[:, 0]))
                    assert torch.equal(d_out[int(offs[k]):int(offs[k + 1])], d_in[int(br[k, 0]):int(br[k, 1])])
                    st, bst = np.array(r3["stages"]), np.array(r3["byte_stages"])
                    line, byte = stats(r3["line"]), stats(r3["byte"])
                    one["run3"][name] = {
                        "ranges": int(lr.shape[0]), "output_bytes": total, "members_read": int(members),
                        "read_lines_ms": line, "read_ranges_equivalent_ms": byte,
                        "ratio_of_medians": round(line["median"] / byte["median"], 3),
                        "lines_stage_ms": {"tiles_locate_select": stats(st[:, 0]), "inflate": stats(st[:, 1]),
                                           "boundary_search": stats(st[:, 2]), "gather": stats(st[:, 3])},
                        "ranges_stage_ms": {"locate_select": stats(bst[:, 0]), "inflate": stats(bst[:, 1]),
                                            "gather": stats(bst[:, 2])}}
                    del d_out
        res["inputs"][which] = one
        del d_comp
    res["note"] = ("build, detour, plain, read_lines, read_ranges: host clock around work that is synchronised at both ends; "
                   "k_ln_count, stages and d2d: HIP events.  GB/s count the inflated bytes once.")
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
