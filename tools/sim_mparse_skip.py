"""CPU model of k_mparse's speculative segment walk at level 1, with and without the step over positions that have no
hash candidate (numpy only, no GPU):  python tools/sim_mparse_skip.py [class] [blocks] [seed]

The model has the kernel's geometry -- passes of 32,768 positions, one lane per 32-position segment, 64 lanes per
wave, guessed entries (the segment's first position; lane 0 knows the true one), a re-walk that lands on a token start
of the lane's previous walk keeps the rest of that walk, rounds of left-neighbour exits until no entry moves, the
hand-back of a pass in which one segment in eight is overshot by two segments -- and ht_matchfinder's search (two
entries per bucket, nice length 32, positions behind n - 5 not searched).  A wave takes as many walk steps as its
slowest lane: the model counts those wave-steps, the re-walks, the rounds and the tokens.  "text" is the bench slab's
generator (synth.text_slab, seed 20250927, its first blocks); every other name is a class of gzp_amd.synth.

The functions are also what tests/l1_skip_cases.py builds and checks its inputs with."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

BLOCK = 65280
HALF, SEG, WAVE = 32768, 32, 64


def lz_hash15(v):
    """The level-1 table's bucket of the four bytes v (little endian), for an array of them."""
    return ((np.asarray(v, dtype=np.uint64) * np.uint64(0x1E35A7BD)) & np.uint64(0xFFFFFFFF)) >> np.uint64(17)


def windows(a):
    """The four bytes at every position p with p + 4 <= n, as little-endian dwords."""
    a = np.asarray(a, dtype=np.uint8).astype(np.uint64)
    return a[:-3] | (a[1:-2] << np.uint64(8)) | (a[2:-1] << np.uint64(16)) | (a[3:] << np.uint64(24))


def buckets(a):
    """The bucket of every hashed position (p + 5 <= n); position 0 is filed under bucket 0."""
    n = len(a)
    h = lz_hash15(windows(a))[:max(n - 4, 0)].astype(np.int64)
    if h.size:
        h[0] = 0
    return h


def d0_of(a):
    """cand[p] of k_candidates: the distance to the previous position of p's bucket, 0 where there is none within
    32,767 bytes or where p is not hashed."""
    n = len(a)
    h = buckets(a)
    d0 = np.zeros(n, dtype=np.int64)
    order = np.argsort(h, kind="stable")
    same = h[order[1:]] == h[order[:-1]]
    d = order[1:] - order[:-1]
    d0[order[1:]] = np.where(same & (d <= 32767), d, 0)
    return d0


class Block:
    def __init__(self, a):
        self.a = np.ascontiguousarray(a, dtype=np.uint8)
        self.n = len(self.a)
        self.d0 = d0_of(self.a)
        self.raw = self.a.tobytes()
        self.memo = {}

    def _extend(self, p, q, max_len):
        x, y = self.a[p:p + max_len], self.a[q:q + max_len]
        ne = np.nonzero(x != y)[0]
        return int(ne[0]) if ne.size else max_len

    def search(self, p):
        """ht_matchfinder_longest_match at p: the match length, 0 for a literal."""
        r = self.memo.get(p)
        if r is not None:
            return r
        n, d0 = self.n, int(self.d0[p])
        best = 0
        if d0 and p + 5 <= n:
            max_len = min(258, n - p)
            nice = min(32, max_len)
            own = self.raw[p:p + 4]
            q0 = p - d0
            if self.raw[q0:q0 + 4] == own:
                best = self._extend(p, q0, max_len)
            r1 = int(self.d0[q0])
            if r1 and d0 + r1 <= 32767 and best < nice:
                q1 = q0 - r1
                if self.raw[q1:q1 + 4] == own:
                    best = max(best, self._extend(p, q1, max_len))
        self.memo[p] = best
        return best

    def parse(self):
        """The sequential greedy parse: (token starts, their lengths; 1 = a literal)."""
        starts, lens = [], []
        p = 0
        while p < self.n:
            ln = self.search(p) or 1
            starts.append(p)
            lens.append(ln)
            p += ln
        return starts, lens


def walk(blk, nz, seg_begin, seg_end, pos, old_marks, old_exit):
    """One lane's walk from pos: (marks, exit, steps).  nz = None: a search at every position; else the set of
    positions that have a candidate, and runs of the others are stepped over without a step of their own."""
    marks, steps = set(), 0
    while pos < seg_end:
        if nz is not None:
            while pos < seg_end and pos not in nz and pos not in old_marks:
                marks.add(pos)
                pos += 1
            if pos >= seg_end:
                break
        if pos in old_marks:  # from here on the two walks are one
            marks |= {m for m in old_marks if m >= pos}
            return marks, old_exit, steps
        steps += 1
        marks.add(pos)
        pos += blk.search(pos) or 1
    return marks, pos, steps


def sim_block(a, skip):
    """The walk of one block: dict of counters, or None when a pass is handed back to the dense kernels."""
    blk = Block(a)
    n = blk.n
    nz = set(np.nonzero(blk.d0[:max(n - 4, 0)])[0].tolist()) if skip else None
    c = dict(first=0, rewalk_steps=0, rewalks=0, rounds=0, tokens=0, lane_steps=0, lane_slots=0, passes=0)
    carry = 0
    for hb in range(0, n, HALF):
        he = min(hb + HALF, n)
        n_seg = (he - hb + SEG - 1) // SEG
        begins = [hb + s * SEG for s in range(n_seg)]
        ends = [min(b + SEG, he) for b in begins]
        entry = [carry] + begins[1:]
        res = [walk(blk, nz, begins[s], ends[s], entry[s], set(), 0) for s in range(n_seg)]
        for w in range(0, n_seg, WAVE):
            st = [r[2] for r in res[w:w + WAVE]]
            c["first"] += max(st)
            c["lane_steps"] += sum(st)
            c["lane_slots"] += max(st) * WAVE
        marks, exits = [r[0] for r in res], [r[1] for r in res]
        if sum(1 for s in range(n_seg) if exits[s] >= ends[s] + 2 * SEG) * 8 > n_seg:
            return None
        c["passes"] += 1
        while True:
            c["rounds"] += 1
            left = exits[:]
            moved = [s for s in range(1, n_seg) if left[s - 1] != entry[s]]
            per_wave = {}
            for s in moved:
                entry[s] = left[s - 1]
                marks[s], exits[s], st = walk(blk, nz, begins[s], ends[s], entry[s], marks[s], exits[s])
                per_wave[s // WAVE] = max(per_wave.get(s // WAVE, 0), st)
            c["rewalks"] += len(moved)
            c["rewalk_steps"] += sum(per_wave.values())
            if not moved:
                break
        c["tokens"] += sum(len(m) for m in marks)
        carry = exits[-1]
    # the walk is the sequential parse
    starts, _ = blk.parse()
    got = sorted(set().union(*marks)) if n <= HALF else None
    assert got is None or got == starts, "the model's walk differs from the sequential parse"
    assert c["tokens"] == len(starts)
    return c


def blocks_of(cls, nblocks, seed):
    from gzp_amd import synth
    if cls == "text":
        a = synth.text_slab(nblocks * BLOCK, seed=20250927 if seed is None else seed)
    else:
        a = synth.make(cls, nblocks * BLOCK, 5 if seed is None else seed)
    return [a[i * BLOCK:(i + 1) * BLOCK] for i in range(nblocks)]


def main():
    cls = sys.argv[1] if len(sys.argv) > 1 else "text"
    nblocks = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    seed = int(sys.argv[3]) if len(sys.argv) > 3 else None
    blocks = blocks_of(cls, nblocks, seed)
    free = np.mean([np.mean(d0_of(b)[:len(b) - 4] == 0) for b in blocks])
    print("%s, %d blocks of %d bytes: %.0f %% of the positions have no candidate" % (cls, nblocks, BLOCK, 100 * free))
    for name, skip in (("today", False), ("with the skip", True)):
        rows = [sim_block(b, skip) for b in blocks]
        kept = [r for r in rows if r is not None]
        if not kept:
            print("%-14s every block is handed back to the dense kernels" % name)
            continue
        k = float(len(kept))
        s = {key: sum(r[key] for r in kept) for key in kept[0]}
        print("%-14s per block: first walks %.0f wave-steps, re-walks %.0f wave-steps (%.0f re-walks), total %.0f; "
              "%.1f rounds per pass; %.0f tokens; lanes %.2f used in the first walks; %d of %d blocks handed back"
              % (name, s["first"] / k, s["rewalk_steps"] / k, s["rewalks"] / k, (s["first"] + s["rewalk_steps"]) / k,
                 s["rounds"] / float(s["passes"]), s["tokens"] / k, s["lane_steps"] / float(max(s["lane_slots"], 1)),
                 len(rows) - len(kept), len(rows)))


if __name__ == "__main__":
    main()
