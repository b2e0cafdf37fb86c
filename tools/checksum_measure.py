"""gzpx_checksum_batch_device on the MI355X beside what it replaces and what it generalises.  bench.py's 550 MiB text
slab resident in HBM; one process, warm, median / min / max of the steps; HIP events around the kernels
(gzpx_dctx_last_check_ms) and the host clock around the call.  The legs of one step run one after the other, so the new
call and the kernels it is compared with alternate.

  (a)  what a caller had before: a device-to-host copy of the slab, then gzpx_crc32_checked / gzpx_adler32_checked over
       it -- against the new call with one entry for the whole slab
  (b)  the (out_offsets, out_sizes) table of the bench stream's members: CRC-32 and Adler-32 by the new call, beside
       k_dcrc32 (the check kernel of a GZIP batch on the WAVE route, where k_lzcopy does not take the CRC) and
       k_dadler32 (the check kernel of a ZLIB batch) over the same bytes
  (c)  balance: the same bytes as one 512 MiB entry plus 64 KiB entries for the rest, and as 64 KiB entries throughout
  (d)  recorded only: a device-to-device copy of the same bytes; CRC-32C on table (b)

Prints one JSON line; --out FILE writes it too.

    python tools/checksum_measure.py [--steps 10] [--warmup 2] [--out profiles/checksum_measure.json]
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
    plain = synth.text_slab(n, seed=20250927)
    d_plain = torch.from_numpy(plain).to("cuda:0")
    with _native.Context(format=_native.FORMAT_BGZF, level=1, buffer_size=65280, max_slab_bytes=n) as c:
        cap = c.slab_bound(n)
        d_comp = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
        comp_len, _ = c.compress_slab_device(d_plain.data_ptr(), n, d_comp.data_ptr(), cap, True)
    comp = d_comp[:comp_len].cpu().numpy()
    d_out = torch.empty(n + 64, dtype=torch.uint8, device="cuda:0")
    h_pinned = torch.empty(n, dtype=torch.uint8).pin_memory()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")

    def clock(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    with _native.DContext(format=_native.FORMAT_BGZF) as d, _native.DContext(format=_native.FORMAT_BGZF) as dw:
        dw.set_route(_native.INFLATE_WAVE)
        offs, sizes, used = d.scan_blocks(comp)
        assert used == comp_len
        nm = offs.size
        ends = offs.astype(np.int64) + sizes.astype(np.int64)
        isz = np.array([struct.unpack("<I", comp[e - 4:e].tobytes())[0] for e in ends], dtype=np.uint32)
        ooff = np.concatenate([[0], np.cumsum(isz.astype(np.uint64))]).astype(np.uint64)
        assert int(ooff[-1]) == n
        member_plain = [plain[int(a):int(b)] for a, b in zip(ooff[:-1], ooff[1:])]
        want_crc = np.array([zlib.crc32(p) for p in member_plain], dtype=np.uint32)
        want_adler = np.array([zlib.adler32(p) for p in member_plain], dtype=np.uint32)
        # a ZLIB batch of the same payloads, for k_dadler32
        parts, z_off, pos = [], [], 0
        for o, s, ad in zip(offs.tolist(), sizes.tolist(), want_adler.tolist()):
            z = b"\x78\x01" + comp[o + 18:o + s - 8].tobytes() + struct.pack(">I", ad)
            parts.append(z)
            z_off.append(pos)
            pos += len(z)
        zblob = b"".join(parts)
        d_z = dev(np.frombuffer(zblob, dtype=np.uint8))
        t_goff, t_gsize = dev(offs.astype(np.uint64)), dev(sizes.astype(np.uint32))
        t_zoff, t_zsize = dev(np.array(z_off, dtype=np.uint64)), dev(np.array([len(z) for z in parts], dtype=np.uint32))
        t_isz, t_ooff = dev(isz), dev(ooff)
        # (c): one 512 MiB entry and 64 KiB entries behind it; 64 KiB entries throughout
        big = 512 << 20
        rest = np.arange(big, n, 65536, dtype=np.uint64)
        c_off = np.concatenate([[0], rest]).astype(np.uint64)
        c_size = np.concatenate([[big], np.minimum(n - rest, 65536)]).astype(np.uint32)
        e_off = np.arange(0, n, 65536, dtype=np.uint64)
        e_size = np.minimum(n - e_off, 65536).astype(np.uint32)
        t_coff, t_csize, t_eoff, t_esize = dev(c_off), dev(c_size), dev(e_off), dev(e_size)
        t_whole = dev(np.array([0, n], dtype=np.uint64))
        sums = torch.zeros(max(nm, e_off.size) + 1, dtype=torch.int32, device="cuda:0")
        p_plain, p_sums = d_plain.data_ptr(), sums.data_ptr()

        def got(k):
            return sums[:k].cpu().numpy().view(np.uint32)

        def new_call(kind, t_off, t_size, k):
            def leg():
                assert d.checksum_batch_device(kind, p_plain, n, t_off.data_ptr(), t_size.data_ptr() if t_size is not None else None,
                                               k, d_sums_ptr=p_sums) == (0, None)
            return leg

        def host_crc32():
            h_pinned.copy_(d_plain)
            host_crc32.value = _native.crc32(h_pinned.numpy())

        def host_adler32():
            h_pinned.copy_(d_plain)
            host_adler32.value = _native.adler32(h_pinned.numpy())

        def parent_dcrc32():
            assert dw.inflate_batch_device(_native.WRAP_GZIP, d_comp.data_ptr(), comp_len, t_goff.data_ptr(), t_gsize.data_ptr(),
                                           None, nm, d_out.data_ptr(), n + 64) == (n, 0)

        def parent_dadler32():
            assert d.inflate_batch_device(_native.WRAP_ZLIB, d_z.data_ptr(), len(zblob), t_zoff.data_ptr(), t_zsize.data_ptr(),
                                          t_isz.data_ptr(), nm, d_out.data_ptr(), n + 64) == (n, 0)

        CRC32, ADLER32, CRC32C = _native.CHECK_CRC32, _native.CHECK_ADLER32, _native.CHECK_CRC32C
        legs = [  # (name, call, the context whose last_check_ms answers for it or None, what step 0 verifies)
            ("a_host_copy_plus_crc32_checked", host_crc32, None, None),
            ("a_new_crc32_one_entry", new_call(CRC32, t_whole, None, 1), d, lambda: got(1)[0] == zlib.crc32(plain)),
            ("a_host_copy_plus_adler32_checked", host_adler32, None, None),
            ("a_new_adler32_one_entry", new_call(ADLER32, t_whole, None, 1), d, lambda: got(1)[0] == zlib.adler32(plain)),
            ("b_new_crc32_member_table", new_call(CRC32, t_ooff, t_isz, nm), d, lambda: (got(nm) == want_crc).all()),
            ("b_parent_k_dcrc32", parent_dcrc32, dw, None),
            ("b_new_adler32_member_table", new_call(ADLER32, t_ooff, t_isz, nm), d, lambda: (got(nm) == want_adler).all()),
            ("b_parent_k_dadler32", parent_dadler32, d, None),
            ("c_new_crc32_512mib_plus_64k", new_call(CRC32, t_coff, t_csize, c_off.size), d,
             lambda: got(2)[1] == zlib.crc32(plain[big:big + 65536])),
            ("c_new_crc32_64k_throughout", new_call(CRC32, t_eoff, t_esize, e_off.size), d,
             lambda: got(1)[0] == zlib.crc32(plain[:65536])),
            ("c_new_adler32_512mib_plus_64k", new_call(ADLER32, t_coff, t_csize, c_off.size), d,
             lambda: got(1)[0] == zlib.adler32(plain[:big])),
            ("c_new_adler32_64k_throughout", new_call(ADLER32, t_eoff, t_esize, e_off.size), d, None),
            ("d_new_crc32c_member_table", new_call(CRC32C, t_ooff, t_isz, nm), d, None),
        ]
        rows = {name: {"call": [], "kernels": []} for name, _, _, _ in legs}
        d2d = []
        for step in range(args.warmup + args.steps):
            for name, fn, ctx, verify in legs:
                t = clock(fn)
                if step == 0 and verify is not None:
                    assert verify(), name
                if step >= args.warmup:
                    rows[name]["call"].append(t)
                    if ctx is not None:
                        rows[name]["kernels"].append(ctx.last_check_ms())
            assert host_crc32.value == zlib.crc32(plain) and host_adler32.value == zlib.adler32(plain) if step == 0 else True
            ev0.record()
            d_out[:n].copy_(d_plain, non_blocking=True)
            ev1.record()
            ev1.synchronize()
            if step >= args.warmup:
                d2d.append(ev0.elapsed_time(ev1))
    res = {"what": "checksum_measure", "build_id": build.source_id(), "device": torch.cuda.get_device_name(0), "bytes": n,
           "members": int(nm), "entries_c": int(c_off.size), "entries_64k": int(e_off.size), "steps": args.steps,
           "warmup": args.warmup, "legs": {}}
    for name, r in rows.items():
        res["legs"][name] = {"call_ms": stats(r["call"])}
        if r["kernels"]:
            k = stats(r["kernels"])
            res["legs"][name]["kernels_ms"] = k
            res["legs"][name]["GB_per_s"] = round(n / (k["median"] / 1e3) / 1e9, 1) if k["median"] > 0 else 0.0
    L = res["legs"]
    for new, old in (("b_new_crc32_member_table", "b_parent_k_dcrc32"), ("b_new_adler32_member_table", "b_parent_k_dadler32")):
        spread = L[old]["kernels_ms"]["max"] - L[old]["kernels_ms"]["min"]
        gap = L[new]["kernels_ms"]["median"] - L[old]["kernels_ms"]["median"]
        L[new]["median_minus_parent_median_ms"] = round(gap, 4)
        L[new]["parent_min_max_spread_ms"] = round(spread, 4)
        L[new]["within_parent_spread"] = bool(gap <= spread)
    for kind in ("crc32", "adler32"):
        b = L["b_new_%s_member_table" % kind]["kernels_ms"]
        gap = L["c_new_%s_512mib_plus_64k" % kind]["kernels_ms"]["median"] - L["c_new_%s_64k_throughout" % kind]["kernels_ms"]["median"]
        L["c_new_%s_512mib_plus_64k" % kind]["median_minus_even_median_ms"] = round(gap, 4)
        L["c_new_%s_512mib_plus_64k" % kind]["within_b_spread"] = bool(gap <= b["max"] - b["min"])
    cp = stats(d2d)
    res["d_d2d_copy_same_bytes"] = {"ms": cp, "GB_per_s": round(n / (cp["median"] / 1e3) / 1e9, 1) if cp["median"] > 0 else 0.0}
    res["note"] = ("call_ms: host clock around a call that is synchronised at both ends.  kernels_ms: HIP events -- for the new call "
                   "its four kernels (plan, tiles, finish, record), for the parent legs the one check kernel of the batch call.  "
                   "GB/s count the hashed bytes once (the copy reads and writes them).")
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
