"""Record what the system's libdeflate.so.0 says to every crafted stream of tests/inflate_cases.py:

    python tests/golden/make_inflate_verdicts.py          (rewrites tests/golden/inflate_verdicts.json)

Per case: its name, the SHA-256 of the raw DEFLATE stream, the room given (the ISIZE its member claims), the return code
of libdeflate_deflate_decompress (0 ok, 1 BAD_DATA, 3 INSUFFICIENT_SPACE) and, for an accepted stream, the bytes (hex;
outputs over 512 bytes by length and SHA-256).  The tests assert against the file, so they need no libdeflate."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))


def render(verdicts):
    return json.dumps({"reference": "libdeflate_deflate_decompress of libdeflate.so.0 (v1.10 behaviour)",
                       "verdicts": verdicts}, indent=1, sort_keys=True) + "\n"


def main():
    import inflate_cases
    ld = inflate_cases.box_libdeflate()
    if ld is None:
        sys.exit("no libdeflate.so.0 on this box")
    with open(inflate_cases.VERDICTS, "w") as f:
        f.write(render(inflate_cases.record(ld)))
    print("wrote %s" % inflate_cases.VERDICTS)


if __name__ == "__main__":
    main()
