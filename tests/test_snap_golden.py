"""tests/golden/snap_vectors.json checked on the CPU: the generator, not the product.  The frame decoder of
snap_cases.py (written from the format description) takes every committed framed stream back to its input and checks
every masked CRC-32C; the restated snappy 1.1.8 loop reproduces the raw vectors; where the snappy binary is present a
sample of raw vectors and framed streams is derived from it once more."""
import pytest

import snap_cases as sc

G = sc.golden()
GEN = sc.generator()


def test_crc32c_check_value():
    assert sc.crc32c(b"123456789") == 0xE3069283
    assert GEN.crc32c(b"123456789") == 0xE3069283
    assert sc.unmask(GEN.mask(0xE3069283)) == 0xE3069283


def test_vectors_cover_the_rules():
    specs = [v["spec"] for v in G["raw"]]
    for n in GEN.RAW_SIZES:
        assert {s[0] for s in specs if s[1] == n and s[0] in GEN.synth.CLASSES} == set(GEN.synth.CLASSES)
    assert {s[3] for s in specs if s[0] == "period"} >= {1, 2, 3}
    assert {s[4] - s[3] for s in specs if s[0] == "echo"} == {2046, 2047, 2048, 2049}
    assert {s[3] for s in specs if s[0] == "literal"} >= {60, 61, 256, 65536}
    bss = {v["spec"][3] for v in G["framed"]}
    assert bss == {32768, 65536, 65537, 131072, 1 << 20}
    assert any(v["size"] == 0 for v in G["framed"])


def test_restated_loop_reproduces_the_raw_vectors():
    """The element rules, one per vector kind, reached by the restated loop (not only its output)."""
    seen = set()
    for v in G["raw"]:
        a = GEN.make_input(v["spec"])[:65536].tobytes()
        if len(a) > 20000 and v["spec"][0] in ("text", "dna", "fastq", "mixed", "lowent", "ascii", "random"):
            continue  # (pure Python: the long inputs of the slow classes are left to the binary leg and the product)
        got = GEN.snappy_raw(a)
        sc.check_digest(got, v, str(v["spec"]))
        assert sc.raw_decode(got) == a
        for tag in _elements(got):
            seen.add(tag)
    assert seen >= {"lit<60", "lit1", "lit2", "copy1", "copy2", "copy2<12"}


def _elements(b):
    pos = 0
    while b[pos] & 0x80:
        pos += 1
    pos += 1
    while pos < len(b):
        tag = b[pos]
        t = tag & 3
        if t == 0:
            m = tag >> 2
            k = m - 59 if m >= 60 else 0
            ln = (int.from_bytes(b[pos + 1:pos + 1 + k], "little") if k else m) + 1
            yield "lit<60" if not k else "lit%d" % k
            pos += 1 + k + ln
        elif t == 1:
            yield "copy1"
            pos += 2
        else:
            yield "copy2<12" if (tag >> 2) + 1 < 12 else "copy2"
            pos += 3


def test_frame_decoder_takes_every_vector_back():
    """Small framed vectors are held whole (hex): decoded to the input, CRCs checked.  Larger ones are framed again
    from the restated loop where that is quick, compared with the digest, and decoded."""
    done = 0
    for v in G["framed"]:
        cls, n, seed, bs = v["spec"]
        a = GEN.make_input([cls, n, seed]).tobytes()
        if "hex" in v:
            got = bytes.fromhex(v["hex"])
        elif n <= 70000:
            got = GEN.frame_stream(a, bs, GEN.snappy_raw)
            sc.check_digest(got, v, str(v["spec"]))
        else:
            continue
        out, chunks = sc.decode_frames(got)
        assert out == a, v["spec"]
        assert chunks == sum(-(-len(a[i:i + bs]) // 65536) for i in range(0, len(a), bs))
        done += 1
    assert done >= 30


def test_sample_rederived_from_the_snappy_binary():
    raw = GEN.load_snappy()
    if raw is None:
        pytest.skip("no snappy binary on this machine (%s)" % GEN.SNAPPY_SO)
    for v in G["raw"][::7]:
        a = GEN.make_input(v["spec"])[:65536].tobytes()
        sc.check_digest(raw(a), v, str(v["spec"]))
    for v in G["framed"][::9]:
        cls, n, seed, bs = v["spec"]
        got = GEN.frame_stream(GEN.make_input([cls, n, seed]).tobytes(), bs, raw)
        sc.check_digest(got, v, str(v["spec"]))
        if n <= 300000:
            assert sc.decode_frames(got)[0] == GEN.make_input([cls, n, seed]).tobytes()
