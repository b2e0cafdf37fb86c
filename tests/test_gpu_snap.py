"""The Snap format on the MI355X (HIP library): every committed vector through the host slab, the device slab (torch
tensors), three submits in flight, encode_block and the twin; bench.py's 550 MiB text slab against its digest; a seeded
sweep of ragged sizes round-tripped through the test's own frame decoder.  Reads tests/golden/snap_vectors.json only."""
import hashlib

import numpy as np
import pytest

import snap_cases as sc
from gzp_amd import _native, synth

pytestmark = pytest.mark.gpu

G = sc.golden()
GEN = sc.generator()


def test_raw_vectors(hip_lib):
    sc.run_raw(hip_lib, G["raw"], GEN)


def test_framed_vectors_host_slab(hip_lib):
    sc.run_framed(hip_lib, G["framed"], GEN)


def test_framed_vectors_device_slab(hip_lib):
    import torch
    for v in G["framed"]:
        cls, n, seed, bs = v["spec"]
        a = GEN.make_input([cls, n, seed])
        with _native.Context(format=_native.FORMAT_SNAP, buffer_size=bs, lib=hip_lib, max_slab_bytes=max(n, 1)) as c:
            cap = c.slab_bound(n)
            d_in = torch.from_numpy(a.copy()).to("cuda:0") if n else torch.empty(1, dtype=torch.uint8, device="cuda:0")
            d_out = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            sizes = np.zeros(c.n_blocks(n), dtype=np.uint32)
            got, nb = c.compress_slab_device(d_in.data_ptr(), n, d_out.data_ptr(), cap, True, block_sizes=sizes)
            out = d_out[:got].cpu().numpy().tobytes()
        sc.check_digest(out, v, "device %s" % v["spec"])
        assert nb == sizes.size and int(sizes.sum()) == got


def test_three_submits_in_flight(hip_lib):
    by_bs = {}
    for v in G["framed"]:
        by_bs.setdefault(v["spec"][3], []).append(v)
    for bs, vs in by_bs.items():
        big = max(v["spec"][1] for v in vs)
        with _native.Context(format=_native.FORMAT_SNAP, buffer_size=bs, lib=hip_lib, max_slab_bytes=max(big, 1)) as c:
            for k in range(0, len(vs), 3):
                group = vs[k:k + 3]
                ins = [GEN.make_input(v["spec"][:3]) for v in group]
                outs = [np.empty(c.slab_bound(a.size), dtype=np.uint8) for a in ins]
                tickets = [c.submit(a.ctypes.data, a.size, o.ctypes.data, o.size, _native.SLAB_FLUSH) for a, o in zip(ins, outs)]
                assert None not in tickets
                for v, o, t in zip(group, outs, tickets):
                    got, _ = c.wait(t)
                    sc.check_digest(o[:got].tobytes(), v, "submit %s" % v["spec"])


def test_encode_block(hip_lib):
    sc.run_encode_block(hip_lib, G["framed"], GEN)


def test_twin(hip_lib):
    sc.run_twin(hip_lib, [v for v in G["framed"] if v["spec"][1] > 0], GEN, batch_blocks=4)
    sc.run_twin_flush(hip_lib, GEN, GEN.snappy_raw, [("random", 300000, 3, 131072), ("zeros", 200000, 4, 65537)])


def test_fullsize_text_slab(hip_lib):
    import torch
    f = G["fullsize"]
    a = synth.text_slab(f["n"], seed=f["seed"])
    with _native.Context(format=_native.FORMAT_SNAP, buffer_size=f["buffer_size"], lib=hip_lib, max_slab_bytes=a.size) as c:
        d_in = torch.from_numpy(a).to("cuda:0")
        cap = c.slab_bound(a.size)
        d_out = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        got, _ = c.compress_slab_device(d_in.data_ptr(), a.size, d_out.data_ptr(), cap, True)
        out = d_out[:got].cpu().numpy()
        host = c.compress_slab(a, True)
    assert got == f["size"]
    assert hashlib.sha256(out.tobytes()).hexdigest() == f["sha256"]
    assert host == out.tobytes()


def test_ragged_sweep_round_trip(hip_lib):
    rng = np.random.default_rng(20261016)
    for _ in range(24):
        bs = int(rng.choice([32768, 65536, 65537, 100000, 131072]))
        n = int(rng.integers(0, 5 * bs))
        cls = str(rng.choice(sorted(synth.CLASSES)))
        a = synth.make(cls, n, int(rng.integers(1, 1000)))
        with _native.Context(format=_native.FORMAT_SNAP, buffer_size=bs, lib=hip_lib, max_slab_bytes=max(n, 1)) as c:
            got, sizes = c.compress_slab(a, _native.SLAB_FLUSH, return_block_sizes=True)
        out, chunks = sc.decode_frames(got)
        assert out == a.tobytes(), (cls, n, bs)
        assert chunks == sum(-(-min(bs, n - i) // 65536) for i in range(0, n, bs))
        assert int(sizes.sum()) == len(got)
