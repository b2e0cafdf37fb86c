"""Reads by range on the MI355X: gzpx_read_ranges_device against what a caller had to do before it existed.
bench.py's 550 MiB text slab, compressed at level 1 on the device and resident in HBM; one process, warm, median /
min / max of the steps.  Three query sets (seed fixed, not tuned):

  (i)   10,000 ranges of 4 KiB at uniformly random offsets
  (ii)  1,000 ranges of 1 MiB
  (iii) one range over the whole stream

and for each:

  new  read_ranges_device (index built once, outside the timer)            host clock, synchronised; its three
                                                                            stages (locate + select, inflate, gather)
                                                                            by HIP events
  (a)  index_device, member selection on the host, decompress_device with
       the host table into a staging tensor, one device-to-device copy
       per range                                                            host clock, synchronised
  (b)  decompress_stream_device of everything, one copy per range           host clock, synchronised
  d2d  one device-to-device copy of the same number of bytes                HIP events

(iii) also reports plain decompress_stream_device: the price of staging + gather.  The per-range copies of (a) and (b)
are torch slice copies, one hipMemcpyAsync each, issued from Python.

Prints one JSON line; --out FILE writes it too.

    python tools/ranges_measure.py [--steps 10] [--warmup 2] [--out FILE]
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
    d_in = torch.from_numpy(synth.text_slab(n, seed=20250927)).to("cuda:0")
    with _native.Context(format=_native.FORMAT_BGZF, level=1, buffer_size=65280, max_slab_bytes=n) as c:
        cap = c.slab_bound(n)
        d_comp = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
        comp_len, _ = c.compress_slab_device(d_in.data_ptr(), n, d_comp.data_ptr(), cap, True)
    rng = np.random.default_rng(20260103)
    sets = {}
    for name, count, length in (("i_10000x4KiB", 10000, 4096), ("ii_1000x1MiB", 1000, 1 << 20), ("iii_whole", 1, n)):
        b = rng.integers(0, n - length + 1, count).astype(np.uint64)
        sets[name] = np.stack([b, b + np.uint64(length)], axis=1)
    d_full = torch.empty(n + 64, dtype=torch.uint8, device="cuda:0")
    d_stage = torch.empty(n + 64, dtype=torch.uint8, device="cuda:0")
    biggest = max(int((r[:, 1] - r[:, 0]).sum()) for r in sets.values())  # (ii) asks for more bytes than the stream holds
    d_out = torch.empty(biggest + 64, dtype=torch.uint8, device="cuda:0")
    d_src = torch.empty(biggest + 64, dtype=torch.uint8, device="cuda:0")  # the source of the plain copy
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    p_comp = d_comp.data_ptr()
    res = {"what": "ranges_measure", "build_id": build.source_id(), "device": torch.cuda.get_device_name(0), "bytes": n,
           "compressed_bytes": int(comp_len), "steps": args.steps, "warmup": args.warmup, "sets": {}}

    def clock(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    with _native.DContext(format=_native.FORMAT_BGZF) as d, d.build_index_device(p_comp, comp_len) as ix:
        res["members"] = ix.n_members
        for name, r in sets.items():
            lens = (r[:, 1] - r[:, 0]).astype(np.int64)
            total = int(lens.sum())
            out_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            begins = r[:, 0].astype(np.int64)

            def new():
                got, _ = d.read_ranges_device(ix, p_comp, comp_len, r, d_out.data_ptr(), d_out.numel())
                assert got == total

            def old_a():
                idx, used, tot = d.index_device(p_comp, comp_len)
                ustart = idx[:, 1].astype(np.int64)
                first = np.searchsorted(ustart, begins, side="right") - 1
                last = np.searchsorted(ustart, begins + lens, side="left") - 1
                mark = np.zeros(ustart.size + 1, dtype=np.int64)
                np.add.at(mark, first, 1)
                np.add.at(mark, last + 1, -1)
                sel = np.nonzero(np.cumsum(mark)[:-1] > 0)[0]
                offs = np.ascontiguousarray(idx[sel, 0])
                ends = np.concatenate([idx[1:, 0], [np.uint64(used)]])
                sizes = np.ascontiguousarray((ends[sel] - offs).astype(np.uint32))
                isz = np.concatenate([ustart[1:], [tot]]) - ustart
                soff = np.zeros(ustart.size, dtype=np.int64)
                soff[sel] = np.cumsum(isz[sel]) - isz[sel]
                d.decompress_device(p_comp, comp_len, offs, sizes, d_stage.data_ptr(), n + 64)
                src = soff[first] + begins - ustart[first]
                for k in range(begins.size):
                    d_out[out_off[k]:out_off[k + 1]].copy_(d_stage[src[k]:src[k] + lens[k]], non_blocking=True)

            def old_b():
                d.decompress_stream_device(p_comp, comp_len, d_full.data_ptr(), n + 64)
                for k in range(begins.size):
                    d_out[out_off[k]:out_off[k + 1]].copy_(d_full[begins[k]:begins[k] + lens[k]], non_blocking=True)

            def plain():
                d.decompress_stream_device(p_comp, comp_len, d_full.data_ptr(), n + 64)

            rows = {"new": [], "a": [], "b": [], "d2d": [], "plain": [], "stages": []}
            for step in range(args.warmup + args.steps):
                keep = step >= args.warmup
                t_new = clock(new)
                st = d.last_ranges_ms()
                members = d.last_ranges_members()
                t_a, t_b = clock(old_a), clock(old_b)
                t_p = clock(plain) if name == "iii_whole" else 0.0
                ev0.record()
                d_out[:total].copy_(d_src[:total], non_blocking=True)
                ev1.record()
                ev1.synchronize()
                if keep:
                    rows["new"].append(t_new)
                    rows["stages"].append(st)
                    rows["a"].append(t_a)
                    rows["b"].append(t_b)
                    rows["plain"].append(t_p)
                    rows["d2d"].append(ev0.elapsed_time(ev1))
            # the new call's bytes against the slab, once, behind the timers
            d.read_ranges_device(ix, p_comp, comp_len, r, d_out.data_ptr(), d_out.numel())
            k = int(np.argmax(lens))
            assert torch.equal(d_out[out_off[k]:out_off[k + 1]], d_in[begins[k]:begins[k] + lens[k]])
            st = np.array(rows["stages"])
            gather = stats(st[:, 2])
            d2d = stats(rows["d2d"])
            one = {"ranges": int(begins.size), "output_bytes": total, "members_read": int(members),
                   "new_read_ranges_ms": stats(rows["new"]),
                   "new_stage_ms": {"locate_select": stats(st[:, 0]), "inflate": stats(st[:, 1]), "gather": gather},
                   "a_index_host_select_blocks_copies_ms": stats(rows["a"]),
                   "b_stream_device_copies_ms": stats(rows["b"]), "d2d_copy_same_bytes_ms": d2d,
                   "gather_GB_per_s": round(total / (gather["median"] / 1e3) / 1e9, 1) if gather["median"] > 0 else 0.0,
                   "d2d_GB_per_s": round(total / (d2d["median"] / 1e3) / 1e9, 1) if d2d["median"] > 0 else 0.0,
                   "new_max_lt_a_min": bool(max(rows["new"]) < min(rows["a"])),
                   "new_max_lt_b_min": bool(max(rows["new"]) < min(rows["b"]))}
            if name == "iii_whole":
                one["plain_stream_device_ms"] = stats(rows["plain"])
                one["price_of_staging_and_gather_ms"] = round(one["new_read_ranges_ms"]["median"] - one["plain_stream_device_ms"]["median"], 4)
            res["sets"][name] = one
    res["note"] = ("new, (a), (b), plain: host clock around work that is synchronised at both ends; stages and d2d: HIP "
                   "events.  GB/s count the output bytes once.  The per-range copies of (a) and (b) are issued from Python.")
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
