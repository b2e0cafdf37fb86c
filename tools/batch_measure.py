"""gzpx_inflate_batch_device on the MI355X against the BGZF path it shares its kernels with.  bench.py's 550 MiB text
slab, compressed at level 1 on the device and resident in HBM; one process, warm, median / min / max of the steps;
HIP events around the kernels and the host clock around the call.

  (a)  decompress_device with the host member table: the path that existed before, on the same bytes -- the yardstick
  (b)  the batch call with the GZIP table over the same stream (device tables, sizes from the footers)
  (c)  the batch call with the RAW table over it (offset + 18, size - 26, ISIZE)
  (d)  a ZLIB batch made on the host by rewrapping every member's payload: 2-byte header, payload, zlib.adler32 of
       zlib's inflate
  (e)  k_dadler32's own time in (d) and its bytes per second, beside a device-to-device copy of the same bytes

Prints one JSON line; --out FILE writes it too.

    python tools/batch_measure.py [--steps 10] [--warmup 2] [--out profiles/batch_measure.json]
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
    d_plain = torch.from_numpy(synth.text_slab(n, seed=20250927)).to("cuda:0")
    with _native.Context(format=_native.FORMAT_BGZF, level=1, buffer_size=65280, max_slab_bytes=n) as c:
        cap = c.slab_bound(n)
        d_comp = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
        comp_len, _ = c.compress_slab_device(d_plain.data_ptr(), n, d_comp.data_ptr(), cap, True)
    comp = d_comp[:comp_len].cpu().numpy()
    d_out = torch.empty(n + 64, dtype=torch.uint8, device="cuda:0")
    d_src = torch.empty(n + 64, dtype=torch.uint8, device="cuda:0")
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

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
        # (d): every member's payload in a zlib wrapper, checksums by zlib
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
        t_goff, t_gsize = dev(offs.astype(np.uint64)), dev(sizes.astype(np.uint32))
        t_roff, t_rsize = dev(offs.astype(np.uint64) + np.uint64(18)), dev((sizes - 26).astype(np.uint32))
        t_zoff, t_zsize = dev(np.array(z_off, dtype=np.uint64)), dev(np.array(z_size, dtype=np.uint32))
        t_isz = dev(isz)
        p_comp = d_comp.data_ptr()

        def leg_a():
            assert d.decompress_device(p_comp, comp_len, offs, sizes, d_out.data_ptr(), n + 64) == n

        def leg_b():
            assert d.inflate_batch_device(_native.WRAP_GZIP, p_comp, comp_len, t_goff.data_ptr(), t_gsize.data_ptr(), None, nm,
                                          d_out.data_ptr(), n + 64) == (n, 0)

        def leg_c():
            assert d.inflate_batch_device(_native.WRAP_RAW, p_comp, comp_len, t_roff.data_ptr(), t_rsize.data_ptr(),
                                          t_isz.data_ptr(), nm, d_out.data_ptr(), n + 64) == (n, 0)

        def leg_d():
            assert d.inflate_batch_device(_native.WRAP_ZLIB, d_z.data_ptr(), len(zblob), t_zoff.data_ptr(), t_zsize.data_ptr(),
                                          t_isz.data_ptr(), nm, d_out.data_ptr(), n + 64) == (n, 0)

        legs = {"a_decompress_device_host_table": leg_a, "b_batch_gzip": leg_b, "c_batch_raw": leg_c, "d_batch_zlib": leg_d}
        rows = {k: {"call": [], "kernels": [], "check": []} for k in legs}
        d2d = []
        for step in range(args.warmup + args.steps):
            for name, fn in legs.items():
                t = clock(fn)
                if step >= args.warmup:
                    rows[name]["call"].append(t)
                    rows[name]["kernels"].append(d.last_inflate_ms())
                    rows[name]["check"].append(d.last_check_ms() if name != "a_decompress_device_host_table" else 0.0)
                assert torch.equal(d_out[:n], d_plain) if step == 0 else True
            ev0.record()
            d_out[:n].copy_(d_src[:n], non_blocking=True)
            ev1.record()
            ev1.synchronize()
            if step >= args.warmup:
                d2d.append(ev0.elapsed_time(ev1))
    res = {"what": "batch_measure", "build_id": build.source_id(), "device": torch.cuda.get_device_name(0), "bytes": n,
           "compressed_bytes": int(comp_len), "members": int(nm), "steps": args.steps, "warmup": args.warmup, "legs": {}}
    for name, r in rows.items():
        k = stats(r["kernels"])
        res["legs"][name] = {"call_ms": stats(r["call"]), "inflate_kernels_ms": k, "check_kernel_ms": stats(r["check"]),
                             "inflate_GiB_per_s": round(n / (k["median"] / 1e3) / 2**30, 1) if k["median"] > 0 else 0.0}
    a = res["legs"]["a_decompress_device_host_table"]["call_ms"]
    for name in ("b_batch_gzip", "c_batch_raw", "d_batch_zlib"):
        m = res["legs"][name]["call_ms"]["median"]
        res["legs"][name]["median_inside_a_min_max"] = bool(a["min"] <= m <= a["max"])
        res["legs"][name]["median_minus_a_median_ms"] = round(m - a["median"], 4)
    ad, cp = stats(rows["d_batch_zlib"]["check"]), stats(d2d)
    res["e_adler"] = {"k_dadler32_ms": ad, "d2d_copy_same_bytes_ms": cp,
                      "k_dadler32_GB_per_s": round(n / (ad["median"] / 1e3) / 1e9, 1) if ad["median"] > 0 else 0.0,
                      "d2d_GB_per_s": round(n / (cp["median"] / 1e3) / 1e9, 1) if cp["median"] > 0 else 0.0}
    res["note"] = ("call_ms: host clock around a call that is synchronised at both ends (leg a copies its table to the device "
                   "inside the call; b, c, d read theirs where it lies).  inflate_kernels_ms, check_kernel_ms, d2d: HIP events.  "
                   "GB/s of (e) count the inflated bytes once (the copy reads and writes them).")
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
