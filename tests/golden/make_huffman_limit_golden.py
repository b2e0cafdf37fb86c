"""Generate tests/golden/huffman_limit_vectors.json: the libdeflate 1.10 binary's output for the inputs of
tests/huffman_limit_cases.py, whose Huffman codes run into their length limits.

Run in the build container only (it needs the libdeflate binary of the image, see make_golden.py):

    python tests/golden/make_huffman_limit_golden.py

Only the inputs come from the cases module (numpy; no oracle, no library).  The raw streams are the binary's, and the
BGZF / Mgzip framing is make_golden.py's restatement of gzp's rules, independent of oracle/gzpx_oracle.c.  Outputs are
stored as size + SHA-256."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import huffman_limit_cases as cases  # noqa: E402
from make_golden import entry, frame_stream, ld_deflate  # noqa: E402


def main():
    raw, streams = [], []
    for name, (make, _, levels) in cases.INPUTS.items():
        a = make()
        for level in levels:
            e = {"name": name, "n": int(a.size), "input_sha256": hashlib.sha256(a.tobytes()).hexdigest(), "level": level}
            e.update(entry(ld_deflate(a, level)))
            e.pop("hex", None)
            raw.append(e)
            for fmt, bs in (("bgzf", cases.BLOCK), ("mgzip", max(int(a.size), cases.BLOCK))):
                if a.size > bs:
                    continue
                st, blk = frame_stream(a, level, fmt, bs)
                e = {"name": name, "fmt": fmt, "buffer_size": bs, "level": level, "block_sizes": blk}
                e.update(entry(st))
                e.pop("hex", None)
                streams.append(e)
    with open(os.path.join(HERE, "huffman_limit_vectors.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_huffman_limit_golden.py",
                   "libdeflate": "v1.10 binary (Ubuntu libdeflate0 1.10-2), compat=1.10",
                   "raw_deflate": raw, "streams": streams}, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print("wrote %d raw, %d stream vectors" % (len(raw), len(streams)))


if __name__ == "__main__":
    main()
