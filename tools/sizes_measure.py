"""gzpx_inflate_batch_sizes_device on the MI355X beside the inflate call it goes in front of.  bench.py's 550 MiB text
slab, compressed at level 1 on the device and resident in HBM (tools/batch_measure.py's stream); one process, warm,
median / min / max of the steps; HIP events around the kernels and the host clock around the synchronised call.

  (a)  the sizes call over the stream's members: as a RAW table (offset + 18, size - 26), as the GZIP table, and over
       the members rewrapped as ZLIB on the host; exact entries, and the RAW / ZLIB tables once more with every entry
       running to the next member's start
  (b)  gzpx_inflate_batch_device on the same tables with the sizes known: kernels, the k_inflate_seg stage, call
  (c)  the workflow for a caller who knows no size -- before: GZPX_BATCH_SHORT_OK with a capacity of 65,536 bytes per
       member (RAW, ZLIB); after: the sizes call plus the fast batch call with the table it wrote, both calls summed
  --passes: one more sizes call per table with the debug clocks on (wave 0's cycles per stage, summed over members)

Prints one JSON line; --out FILE writes it too.

    python tools/sizes_measure.py [--steps 10] [--warmup 2] [--passes] [--out profiles/sizes_measure.json]
"""
import argparse
import json
import os
import struct
import sys
import time
import zlib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from gzp_amd import _native, build, synth  # noqa: E402

CAPACITY = 65536  # (c) before: what a caller who knows only "BGZF-sized" can give every member


def stats(ms):
    return {"median": round(float(np.median(ms)), 4), "min": round(float(min(ms)), 4), "max": round(float(max(ms)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bytes", type=int, default=576_716_800)
    ap.add_argument("--passes", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    n = args.bytes
    d_plain = torch.from_numpy(synth.text_slab(n, seed=20250927)).to("cuda:0")
    with _native.Context(format=_native.FORMAT_BGZF, level=1, buffer_size=65280, max_slab_bytes=n) as c:
        cap = c.slab_bound(n)
        d_comp = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
        comp_len, _ = c.compress_slab_device(d_plain.data_ptr(), n, d_comp.data_ptr(), cap, True)
    comp = d_comp[:comp_len].cpu().numpy()

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")

    def clock(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    with _native.DContext(format=_native.FORMAT_BGZF) as d:
        offs, sizes, used = d.scan_blocks(comp)
        assert used == comp_len
        nm = offs.size
        ends = offs.astype(np.int64) + sizes.astype(np.int64)
        isz = np.array([struct.unpack("<I", comp[e - 4:e].tobytes())[0] for e in ends], dtype=np.uint32)
        parts, z_off, z_size, pos = [], [], [], 0
        for o, s in zip(offs.tolist(), sizes.tolist()):
            m = comp[o:o + s].tobytes()
            z = b"\x78\x01" + m[18:-8] + struct.pack(">I", zlib.adler32(zlib.decompress(m, 31)))
            parts.append(z)
            z_off.append(pos)
            z_size.append(len(z))
            pos += len(z)
        zblob = b"".join(parts)
        d_z = dev(np.frombuffer(zblob, dtype=np.uint8))
        p_comp = d_comp.data_ptr()
        r_off = offs.astype(np.uint64) + np.uint64(18)
        r_loose = np.append(r_off[1:], np.uint64(comp_len)) - r_off  # to the next member's payload, or the stream's end
        z_offa = np.array(z_off, dtype=np.uint64)
        z_loose = np.append(z_offa[1:], np.uint64(len(zblob))) - z_offa
        # name -> (wrap, input pointer, input length, offsets, sizes, the member lengths the sizes call must find)
        tables = {
            "raw": (_native.WRAP_RAW, p_comp, comp_len, dev(r_off), dev((sizes - 26).astype(np.uint32)), None),
            "gzip": (_native.WRAP_GZIP, p_comp, comp_len, dev(offs.astype(np.uint64)), dev(sizes.astype(np.uint32)), sizes),
            "zlib": (_native.WRAP_ZLIB, d_z.data_ptr(), len(zblob), dev(z_offa), dev(np.array(z_size, dtype=np.uint32)),
                     np.array(z_size, dtype=np.uint32)),
            "raw_loose": (_native.WRAP_RAW, p_comp, comp_len, dev(r_off), dev(r_loose.astype(np.uint32)), None),
            "zlib_loose": (_native.WRAP_ZLIB, d_z.data_ptr(), len(zblob), dev(z_offa), dev(z_loose.astype(np.uint32)),
                           np.array(z_size, dtype=np.uint32)),
        }
        t_isz = dev(isz)
        t_osz = torch.zeros(nm, dtype=torch.int32, device="cuda:0")
        t_used = torch.zeros(nm, dtype=torch.int32, device="cuda:0")
        t_cap = dev(np.full(nm, CAPACITY, dtype=np.uint32))
        d_out = torch.empty(max(n + 64, nm * CAPACITY), dtype=torch.uint8, device="cuda:0")

        def sizes_call(name):
            w, p, ln, to, ts, _ = tables[name]
            assert d.inflate_batch_sizes_device(w, p, ln, to.data_ptr(), ts.data_ptr(), nm, t_osz.data_ptr(), t_used.data_ptr()) == (n, 0)

        def batch_call(name, osz=None, in_sizes=None):
            w, p, ln, to, ts, _ = tables[name]
            assert d.inflate_batch_device(w, p, ln, to.data_ptr(), (in_sizes if in_sizes is not None else ts).data_ptr(),
                                          (osz if osz is not None else t_isz).data_ptr(), nm, d_out.data_ptr(), n + 64) == (n, 0)

        def short_ok_call(name):
            w, p, ln, to, ts, _ = tables[name]
            got = d.inflate_batch_device(w, p, ln, to.data_ptr(), ts.data_ptr(), t_cap.data_ptr(), nm, d_out.data_ptr(),
                                         nm * CAPACITY, short_ok=True)
            assert got == (nm * CAPACITY, 0)

        # what the sizes call answers is checked once per table against the footers and the members' lengths
        for name, (w, p, ln, to, ts, lens) in tables.items():
            sizes_call(name)
            assert np.array_equal(t_osz.cpu().numpy().view(np.uint32), isz), name
            if lens is not None:
                assert np.array_equal(t_used.cpu().numpy().view(np.uint32), lens.astype(np.uint32)), name
        batch_call("raw")
        assert torch.equal(d_out[:n], d_plain)

        legs = {}
        for name in tables:
            legs["a_sizes_" + name] = (lambda nm_=name: sizes_call(nm_))
        for name in ("raw", "gzip", "zlib"):
            legs["b_batch_" + name] = (lambda nm_=name: batch_call(nm_))
        for name in ("raw", "zlib"):
            legs["c_before_short_ok_" + name] = (lambda nm_=name: short_ok_call(nm_))
        rows = {k: {"call": [], "kernels": [], "seg": [], "redo": []} for k in legs}
        after = {name: [] for name in ("raw", "zlib", "zlib_loose")}
        for step in range(args.warmup + args.steps):
            for name, fn in legs.items():
                t = clock(fn)
                if step >= args.warmup:
                    rows[name]["call"].append(t)
                    rows[name]["kernels"].append(d.last_inflate_ms())
                    rows[name]["seg"].append(d.last_inflate_stage_ms()[0])
                    rows[name]["redo"].append(d.last_redo_count())
            for name in after:  # (c) after: the two calls of the workflow back to back, the second fed by the first
                def both(nm_=name):
                    sizes_call(nm_)
                    batch_call(nm_, osz=t_osz, in_sizes=t_used if nm_.endswith("_loose") else None)
                t = clock(both)
                if step >= args.warmup:
                    after[name].append(t)
        assert torch.equal(d_out[:n], d_plain)
        passes = {}
        if args.passes:  # DBlock.cyc of the count-only k_inflate_seg, summed over the members (wave 0's clocks)
            keys = ("member", "headers_tables", "pass1", "pass2", "pass3", "spans", "pass2_iterations", "symbol_steps")
            d.debug_inflate(1)
            for name in ("raw", "zlib"):
                sizes_call(name)
                passes["sizes_" + name] = dict(zip(keys, d.debug_inflate(1)))
                batch_call(name)
                passes["batch_" + name] = dict(zip(keys, d.debug_inflate(1)))
            d.debug_inflate(0)
    res = {"what": "sizes_measure", "build_id": build.source_id(), "device": torch.cuda.get_device_name(0), "bytes": n,
           "compressed_bytes": int(comp_len), "members": int(nm), "steps": args.steps, "warmup": args.warmup,
           "short_ok_capacity": CAPACITY, "legs": {}}
    for name, r in rows.items():
        k = stats(r["kernels"])
        res["legs"][name] = {"call_ms": stats(r["call"]), "inflate_kernels_ms": k, "k_inflate_seg_ms": stats(r["seg"]),
                             "handed_back": int(max(r["redo"])),
                             "MiB_per_s_of_output": round(n / (k["median"] / 1e3) / 2**20, 0) if k["median"] > 0 else 0.0}
    res["c_unknown_sizes"] = {}
    for name, ts in after.items():
        row = {"after_sizes_plus_batch_call_ms": stats(ts)}
        before = "c_before_short_ok_" + name
        if before in rows:
            row["before_short_ok_call_ms"] = stats(rows[before]["call"])
            row["after_max_below_before_min"] = bool(max(ts) < min(rows[before]["call"]))
        res["c_unknown_sizes"][name] = row
    if passes:
        res["debug_clocks"] = passes
    res["note"] = ("call_ms: host clock around a call that is synchronised at both ends.  inflate_kernels_ms: HIP events around "
                   "the inflate kernels (sizes: the count-only ones); k_inflate_seg_ms: its first stage.  *_loose: every entry "
                   "runs to the next member's start; a loose ZLIB table has no 'before' (SHORT_OK needs exact entries).")
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
