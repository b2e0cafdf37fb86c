#!/usr/bin/env python3
"""Are kernels the same machine code in two builds?  Takes two assembly listings of gzpx_kernels.hip for gfx950

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include --cuda-device-only -S gzp_amd/csrc/gzpx_kernels.hip -o X.s

and compares, for every function whose mangled name matches --match and not --skip, its instructions (local labels
renumbered: their numbers count the functions in front) and its resource lines (the .amdhsa_kernel block and the
"; NumSgprs / NumVgprs / ScratchSize / Occupancy / LDSByteSize ..." comments).  Exit status 0: all the same.

    tools/isa_same.py parent.s branch.s --match 'k_inflate|k_lzcopy|seg_' --skip 'ILb1'

(--skip 'ILb1': instances whose first template argument, DBG, is true.)"""
import argparse
import re
import sys

LABEL = re.compile(r"\.L(BB|func_begin|func_end|tmp|JTI)(\d+)")


def functions(path):
    """{symbol: [normalised lines]} of the listing: code from `symbol:` to its .Lfunc_end, and the kernel descriptor."""
    out, cur, name = {}, None, None
    desc = None
    with open(path, errors="replace") as f:
        for raw in f:
            line = raw.rstrip()
            m = re.match(r"^([A-Za-z_][\w$.]*):\s*(;.*)?$", line)
            if m and not line.startswith(".L") and cur is None:
                name, cur = m.group(1), []
                continue
            if cur is not None:
                s = line.strip()
                if s.startswith(".Lfunc_end"):
                    out.setdefault(name, []).extend(cur)
                    cur = None
                    continue
                if not s or s.startswith(("; %bb", "; =>", "; in Loop", "; Parent Loop", ";   in Loop", "; Child Loop", ";   Child Loop", ";     Child Loop")):
                    continue
                if s.startswith(";") and not re.match(r"; (NumSgprs|NumVgprs|NumAgprs|TotalNumVgprs|ScratchSize|Occupancy|LDSByteSize|SGPRBlocks|VGPRBlocks|codeLenInByte|NumSGPRsForWavesPerEU|NumVGPRsForWavesPerEU|AccumOffset|MemoryBound|WaveLimiterHint)", s):
                    continue
                s = re.sub(r"\s*;.*$", "", s) if not s.startswith(";") else s
                cur.append(LABEL.sub(lambda k: ".L%s#" % k.group(1), s))
                continue
            m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", line)
            if m:
                desc = (m.group(1), [])
                continue
            if desc is not None:
                if line.strip() == ".end_amdhsa_kernel":
                    out.setdefault(desc[0], []).extend(["[descriptor]"] + desc[1])
                    desc = None
                else:
                    desc[1].append(line.strip())
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--match", required=True)
    ap.add_argument("--skip", default=None)
    args = ap.parse_args()
    fa, fb = functions(args.a), functions(args.b)
    want = lambda n: re.search(args.match, n) and not (args.skip and re.search(args.skip, n))
    names = sorted(n for n in set(fa) | set(fb) if want(n))
    if not names:
        print("no function matches")
        return 2
    differ = 0
    for n in names:
        if n not in fa or n not in fb:
            print("ONLY IN %s  %s" % (args.a if n in fa else args.b, n))
            differ += 1
        elif fa[n] != fb[n]:
            k = next((i for i, (x, y) in enumerate(zip(fa[n], fb[n])) if x != y), min(len(fa[n]), len(fb[n])))
            print("DIFFERS     %s\n    line %d of %d / %d:  %r  |  %r" % (n, k, len(fa[n]), len(fb[n]), fa[n][k:k + 1], fb[n][k:k + 1]))
            differ += 1
        else:
            print("same  %6d lines  %s" % (len(fa[n]), n))
    print("%d functions compared, %d differ" % (len(names), differ))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
