"""Record what the system's libdeflate.so.0 says to the wrapped members of tests/batch_cases.py:

    python tests/golden/make_wrap_verdicts.py          (rewrites tests/golden/wrap_verdicts.json)

Per case: its name, the wrapper, the SHA-256 of the member, the room given and the return code of
libdeflate_gzip_decompress / libdeflate_zlib_decompress / libdeflate_deflate_decompress without actual_out_nbytes_ret
(0 ok, 1 BAD_DATA, 2 SHORT_OUTPUT, 3 INSUFFICIENT_SPACE).  The tests assert against the file, so they need no
libdeflate."""
import ctypes
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))


def box_libdeflate():
    for path in ("libdeflate.so.0", "/lib/x86_64-linux-gnu/libdeflate.so.0", "/usr/lib/x86_64-linux-gnu/libdeflate.so.0",
                 "/usr/lib64/libdeflate.so.0"):
        try:
            L = ctypes.CDLL(path)
        except OSError:
            continue
        L.libdeflate_alloc_decompressor.restype = ctypes.c_void_p
        calls = []
        for name in ("libdeflate_deflate_decompress", "libdeflate_zlib_decompress", "libdeflate_gzip_decompress"):
            f = getattr(L, name)
            f.restype = ctypes.c_int
            f.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
            calls.append(f)
        d = L.libdeflate_alloc_decompressor()

        def verdict(wrap, member, room):
            out = ctypes.create_string_buffer(max(room, 1))
            return calls[wrap](d, bytes(member), len(member), out, room, None)
        return verdict
    return None


def main():
    import batch_cases
    verdict = box_libdeflate()
    if verdict is None:
        sys.exit("no libdeflate.so.0 on this box")
    rows = [{"case": name, "wrap": wrap, "sha256": hashlib.sha256(m).hexdigest(), "room": room, "rc": verdict(wrap, m, room)}
            for name, wrap, m, room in batch_cases.recorded_cases()]
    assert len({r["case"] for r in rows}) == len(rows)
    with open(batch_cases.VERDICTS, "w") as f:
        f.write(json.dumps({"reference": "libdeflate_{deflate,zlib,gzip}_decompress of libdeflate.so.0 (v1.10 behaviour)",
                            "verdicts": rows}, indent=1, sort_keys=True) + "\n")
    print("wrote %s (%d cases)" % (batch_cases.VERDICTS, len(rows)))


if __name__ == "__main__":
    main()
