"""Member discovery on the MI355X: what it costs to inflate a BGZF stream that lies in HBM with nobody having walked
its headers, against the host detour it replaces.  bench.py's 550 MiB text slab, compressed at level 1 on the device
and never copied to the host; one process, warm, median / min / max of the steps:

  (a) decompress_stream_device                 scan + inflate, nothing on the host             host clock, synchronised
  (b) decompress_device, tables made before    the inflate alone                               HIP events
  (c) what (a) replaces, all inside the timer  D2H of the stream into page-locked memory +
                                               gzpx_scan_blocks + (b)                          host clock, synchronised
  (d) the scan kernels alone                   gzpx_dctx_last_scan_ms, and the bytes they      HIP events
                                               read / (d) next to the HBM roofline

Prints one JSON line; --out FILE writes it too.

    python tools/scan_measure.py [--steps 10] [--warmup 2] [--out FILE]
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

MIB = 1 << 20
HBM_ROOFLINE_GB_S = 8000.0  # MI355X data sheet: 8 TB/s


def stats(ms):
    return {"median": round(float(np.median(ms)), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


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
    d_out = torch.empty(n + 64, dtype=torch.uint8, device="cuda:0")
    pinned = torch.empty(comp_len, dtype=torch.uint8).pin_memory()
    host = pinned.numpy()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a_ms, b_ms, c_ms, d_ms, c_parts = [], [], [], [], []
    with _native.DContext(format=_native.FORMAT_BGZF) as d:
        # the tables of (b), made outside every timer
        pinned.copy_(d_comp[:comp_len])
        offs, sizes, used = d.scan_blocks(host)
        assert used == comp_len
        for step in range(args.warmup + args.steps):
            keep = step >= args.warmup
            # (a)
            torch.cuda.synchronize()
            t = time.perf_counter()
            got, nb, consumed = d.decompress_stream_device(d_comp.data_ptr(), comp_len, d_out.data_ptr(), n + 64)
            dt = (time.perf_counter() - t) * 1e3
            assert (got, nb, consumed) == (n, offs.size, comp_len)
            if keep:
                a_ms.append(dt)
                d_ms.append(d.last_scan_ms())
            # (b)
            ev0.record()
            d.decompress_device(d_comp.data_ptr(), comp_len, offs, sizes, d_out.data_ptr(), n + 64)
            ev1.record()
            ev1.synchronize()
            if keep:
                b_ms.append(ev0.elapsed_time(ev1))
            # (c)
            torch.cuda.synchronize()
            t = time.perf_counter()
            pinned.copy_(d_comp[:comp_len])
            t1 = time.perf_counter()
            o2, s2, u2 = d.scan_blocks(host)
            t2 = time.perf_counter()
            d.decompress_device(d_comp.data_ptr(), comp_len, o2, s2, d_out.data_ptr(), n + 64)
            t3 = time.perf_counter()
            if keep:
                c_ms.append((t3 - t) * 1e3)
                c_parts.append(((t1 - t) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
        assert torch.equal(d_out[:n], d_in)
    a, b, cc, dd = stats(a_ms), stats(b_ms), stats(c_ms), stats(d_ms)
    parts = np.median(np.array(c_parts), axis=0)
    scan_gb_s = comp_len / (dd["median"] / 1e3) / 1e9 if dd["median"] > 0 else 0.0
    res = {"what": "scan_measure", "build_id": build.source_id(), "device": torch.cuda.get_device_name(0),
           "bytes": n, "compressed_bytes": int(comp_len), "members": int(offs.size), "steps": args.steps,
           "warmup": args.warmup,
           "a_stream_device_ms": a, "b_inflate_host_tables_ms": b, "c_host_detour_ms": cc,
           "c_parts_ms_median": {"d2h_pinned": round(float(parts[0]), 4), "gzpx_scan_blocks": round(float(parts[1]), 4),
                                 "decompress_device": round(float(parts[2]), 4)},
           "d_scan_kernels_ms": dd,
           "a_lt_c": bool(a["median"] < cc["median"]), "a_max_lt_c_min": bool(a["max"] < cc["min"]),
           "price_of_discovery_ms": round(a["median"] - b["median"], 4),
           "scan_stream_GB_per_s": round(scan_gb_s, 1),
           "scan_pct_of_hbm_roofline": round(100.0 * scan_gb_s / HBM_ROOFLINE_GB_S, 2),
           "note": "(a), (c): host clock around calls that return synchronised; (b), (d): HIP events.  "
                   "scan_stream_GB_per_s counts the stream once (the one-read bound); the write pass rereads the "
                   "segments that hold candidates."}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
