"""GPU: bt_flow_table_device (beatrice_amd/csrc/bt_flowtab.hip), the flow table of a
device-resident batch: flow ids and flow records. Expected values come from the restatement in
flowtab_ref.py (a dict over (class, key bytes), the keys from the goldens' reference-made bt_rec or
from the Python layer walk), never from the code under test. Every output, and the scratch, sits
in a poisoned buffer between two 256-byte guards and is compared whole."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flow_ref as fr  # noqa: E402
import flowtab_ref as ftr  # noqa: E402
from beatrice_amd import abi  # noqa: E402
from conftest import load_golden  # noqa: E402

pytestmark = pytest.mark.gpu

POISON = 0xC7
GUARD = 256
SIZES = [0, 1, 63, 64, 65, 16383, 16384, 16385, 3 * 16384 + 17]
SOURCES = ["c3", "c4", "fuzz", "edge"]
FORMATS = ["packed", "xdp", "stride"]
STRIDE = 256   # fixed-stride sources: every frame cut or zero-padded to this


class Guarded:
    """`size` bytes on the device between two guards, all poisoned."""

    def __init__(self, ctx, size):
        self.ctx, self.size = ctx, size
        self.buf = ctx.alloc(GUARD + (size + 7) // 8 * 8 + GUARD)
        self.ptr = self.buf.ptr + GUARD
        assert self.ptr % 256 == 0
        abi._check(abi.lib().bt_memset_d(ctx.h, self.buf.ptr, POISON, self.buf.nbytes))

    def read(self, dtype=np.uint8):
        full = self.buf.download(np.zeros(self.buf.nbytes, np.uint8))
        assert (full[:GUARD] == POISON).all() and (full[GUARD + self.size:] == POISON).all(), "guard bytes written"
        return full[GUARD:GUARD + self.size].copy().view(dtype)

    def free(self):
        self.buf.free()


@functools.lru_cache(maxsize=None)
def strided(name):
    """A golden's frames cut or zero-padded to STRIDE bytes: (the bytes, flow_ref's key triple by the Python walk)."""
    g, _ = load_golden(name)
    off, ln = (g["desc"] & fr.MASK48).astype(np.int64), (g["desc"] >> np.uint64(48)).astype(np.int64)
    data = np.zeros((len(off), STRIDE), np.uint8)
    for k, (o, m) in enumerate(zip(off, np.minimum(ln, STRIDE))):
        data[k, :m] = g["data"][o:o + m]
    return data, {l3: fr.key_of_frames([r.tobytes() for r in data], l3) for l3 in (False, True)}


@functools.lru_cache(maxsize=None)
def golden_keys(name, l3_only=False):
    g, _ = load_golden(name)
    return fr.key_of_rec(g["rec"], l3_only)


class Source:
    """n frames of a golden (repeated) on the device as packed or XDP descriptors or at a fixed
    stride; or crafted data / descriptors."""

    def __init__(self, ctx, name, n, fmt="packed", data=None, desc=None, nbytes=None):
        g, _ = load_golden(name)
        self.name, self.n, self.fmt, self.crafted = name, n, fmt, data is not None
        base = g["desc"] if desc is None else desc
        self.reps = np.resize(np.arange(len(base)), n) if n else np.zeros(0, np.int64)
        self.d_desc = None
        if fmt == "stride":
            rows, _ = strided(name)
            host = rows[self.reps].reshape(-1) if n else np.zeros(0, np.uint8)
            self.lens = np.full(n, STRIDE, np.int64)
            self.d_data = ctx.alloc(max(256, len(host)))
            if len(host):
                self.d_data.upload(host)
            self.batch = abi.Batch(self.d_data.ptr, None, STRIDE, n, 0, 0, 0)
            return
        data = g["data"] if data is None else data
        self.desc = np.resize(base, n).astype(np.uint64) if n else np.zeros(0, np.uint64)
        self.lens = (self.desc >> np.uint64(48)).astype(np.int64)
        self.d_data = ctx.alloc(len(data) + 256)
        self.d_data.zero()
        self.d_data.upload(data)
        up = self.desc
        if fmt == "xdp":   # struct xdp_desc {u64 addr; u32 len; u32 options}
            x = np.zeros((max(n, 1), 2), np.uint64)
            x[:n, 0] = self.desc & fr.MASK48
            x[:n, 1] = self.desc >> np.uint64(48) | np.uint64(0xABCD0000 << 32)
            up = x.reshape(-1)
        self.d_desc = ctx.alloc(max(16, up.nbytes))
        if up.nbytes:
            self.d_desc.upload(up)
        self.batch = abi.Batch(self.d_data.ptr, self.d_desc.ptr, 0, n, len(data) if nbytes is None else nbytes,
                               abi.DESC_XDP if fmt == "xdp" else abi.DESC_PACKED, 0)

    def want(self, flags=0, select=None, flow_cap=None, slots=0):
        """The restatement's outputs for this source (goldens only)."""
        l3 = bool(flags & ftr.L3_ONLY)
        inputs, nbytes, klass = strided(self.name)[1][l3] if self.fmt == "stride" else golden_keys(self.name, l3)
        return ftr.expected(inputs[self.reps], nbytes[self.reps], klass[self.reps], self.lens, flags, select, flow_cap, slots)

    def free(self):
        self.d_data.free()
        if self.d_desc:
            self.d_desc.free()


def select_words(kind, n, seed=0):
    """Verdict-layout words of a selection, with garbage in the last word's bits at or above n."""
    ntiles = (n + 63) // 64
    if kind == "null" or ntiles == 0:
        return None
    rng = np.random.default_rng(seed + n)
    if kind == "ones":
        w = np.full(ntiles, ~np.uint64(0))
    elif kind == "zeros":
        w = np.zeros(ntiles, np.uint64)
    else:
        w = rng.integers(0, 1 << 63, ntiles, dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, ntiles, dtype=np.uint64)
    if n % 64:
        w = w.copy()
        w[-1] |= ~np.uint64(0) << np.uint64(n % 64)   # must be ignored
    return w


def run(ctx, batch, n, want, flags=0, select=None, flow_cap=None, slots=0, stream=None, d_select=None, where="",
        overflow=False):
    """One call into poisoned, guarded buffers (scratch included); flow_id, flows and *result
    against `want`, whole. flow_cap None: room for every packet. Returns the raw outputs."""
    cap = n if flow_cap is None else flow_cap
    need = abi.flow_table_scratch_bytes(n, slots)
    bufs = {"flow_id": Guarded(ctx, 4 * n), "flows": Guarded(ctx, 80 * cap), "result": Guarded(ctx, 72),
            "scratch": Guarded(ctx, need)}
    d_sel = None
    if select is not None and d_select is None:
        d_sel = ctx.alloc(max(16, select.nbytes))
        d_sel.upload(select)
    try:
        ctx.flow_table_device(batch, abi.FlowTableOpts(flags, slots, cap, 0), bufs["scratch"].ptr, need, bufs["result"].ptr,
                              select=d_select if d_select is not None else d_sel, flow_id=bufs["flow_id"].ptr,
                              flows=bufs["flows"].ptr if cap else None, stream=stream)
        if stream is not None:
            ctx.stream_synchronize(stream)
        ctx.synchronize()
        raw = {k: bufs[k].read() for k in ("flow_id", "flows", "result")}
        bufs["scratch"].read()   # its guards
        res = abi.FlowTableResult.from_bytes(raw["result"]).as_dict()
        if overflow:
            return res
        assert res == want["result"], f"{where}: result " + ", ".join(k for k in res if res[k] != want["result"][k])
        fid = raw["flow_id"].view(np.uint32)
        bad = np.nonzero(fid != want["flow_id"])[0]
        assert len(bad) == 0, f"{where}: flow_id differs at {bad[:8]}: {fid[bad[:8]]} != {want['flow_id'][bad[:8]]}"
        nw = res["n_written"]
        assert raw["flows"][:80 * nw].tobytes() == want["flows"].tobytes(), f"{where}: flows"
        assert (raw["flows"][80 * nw:] == POISON).all(), f"{where}: flows written at or past n_written"
        return raw
    finally:
        for b in list(bufs.values()) + ([d_sel] if d_sel else []):
            b.free()


@pytest.mark.parametrize("n", SIZES)
def test_sizes_at_tile_and_chunk_edges(gpu_ctx, n):
    """Every source at every size; the format and the flags rotate, so that every source meets every format."""
    si = SIZES.index(n)
    for k, name in enumerate(SOURCES):
        fmt = FORMATS[(si + k) % 3]
        flags = (0, ftr.BIDIRECTIONAL, ftr.L3_ONLY, ftr.L3_ONLY | ftr.BIDIRECTIONAL)[(si + k) % 4]
        sel = select_words(("null", "random")[(si + k) % 2], n)
        src = Source(gpu_ctx, name, n, fmt)
        try:
            run(gpu_ctx, src.batch, n, src.want(flags, sel), flags, sel, where=f"{name} {fmt} n={n} flags={flags}")
        finally:
            src.free()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", SOURCES)
def test_sources_in_every_format(gpu_ctx, name, fmt):
    """Each golden repeated two and a half times: every flow has several packets. Both flags, four selections."""
    g, _ = load_golden(name)
    n = len(g["desc"]) * 5 // 2
    src = Source(gpu_ctx, name, n, fmt)
    try:
        for flags, kind in ((0, "null"), (ftr.BIDIRECTIONAL, "random"), (ftr.L3_ONLY, "ones"),
                            (ftr.L3_ONLY | ftr.BIDIRECTIONAL, "random"), (0, "zeros")):
            sel = select_words(kind, n, seed=flags)
            want = src.want(flags, sel)
            if kind != "zeros":
                assert 0 < want["result"]["n_flows"] < want["result"]["n_selected"]
            run(gpu_ctx, src.batch, n, want, flags, sel, where=f"{name} {fmt} flags={flags} {kind}")
    finally:
        src.free()


def _tcp(src, dst, sp, dp):
    ip = bytes([0x45, 0, 0, 40, 0, 0, 0, 0, 64, 6, 0, 0]) + bytes(src) + bytes(dst)
    return bytes(12) + b"\x08\x00" + ip + sp.to_bytes(2, "big") + dp.to_bytes(2, "big") + bytes(16)


def _crafted(ctx, frames, n, nbytes=None):
    """n descriptors over the frames (repeated in order), each frame at an odd offset."""
    data, offs = bytearray(), []
    for f in frames:
        data += bytes(-len(data) % 4 + 1)   # the next frame starts at 1 mod 4
        offs.append(len(data))
        data += f
    desc = np.array([o | len(f) << 48 for o, f in zip(offs, frames)], np.uint64)
    # with nbytes, only that much is uploaded: the device buffer holds zeros behind it
    return Source(ctx, "c3", n, data=np.frombuffer(bytes(data), np.uint8)[:nbytes], desc=desc, nbytes=nbytes)


def crafted_want(src, frames, flags=0, **kw):
    """The restatement over a _crafted source: the Python walk of the distinct frames, repeated as the descriptors are."""
    inputs, nbytes, klass = fr.key_of_frames(frames, bool(flags & ftr.L3_ONLY))
    return ftr.expected(inputs[src.reps], nbytes[src.reps], klass[src.reps], src.lens, flags, **kw)


def test_one_flow_is_maximum_contention_on_one_slot(gpu_ctx):
    n = 3 * 16384 + 17
    fwd, rev = _tcp([10, 1, 2, 3], [10, 3, 2, 1], 40000, 443), _tcp([10, 3, 2, 1], [10, 1, 2, 3], 443, 40000)
    src = _crafted(gpu_ctx, [fwd], n)
    try:
        want = crafted_want(src, [fwd])
        assert want["result"]["n_flows"] == 1 and want["flows"]["packets"].tolist() == [[n, 0]]
        assert want["flows"]["last"].tolist() == [n - 1] and want["flows"]["bytes"].tolist() == [[54 * n, 0]]
        run(gpu_ctx, src.batch, n, want, where="one flow")
        run(gpu_ctx, src.batch, n, crafted_want(src, [fwd], slots=128), slots=128, where="one flow, 128 slots")
    finally:
        src.free()
    src = _crafted(gpu_ctx, [fwd, rev, rev], n)   # both directions of it
    try:
        want = crafted_want(src, [fwd, rev, rev], ftr.BIDIRECTIONAL)
        assert want["result"]["n_flows"] == 1 and min(want["flows"]["packets"][0]) > 16384
        run(gpu_ctx, src.batch, n, want, ftr.BIDIRECTIONAL, where="one conversation")
    finally:
        src.free()


def test_every_packet_its_own_flow(gpu_ctx):
    g, _ = load_golden("c1")
    n = len(g["rec"])
    assert n == 10000 and len(g["data"]) == 64 * n
    d = gpu_ctx.alloc(64 * n)
    try:
        d.upload(g["data"])
        inputs, nbytes, klass = golden_keys("c1")
        want = ftr.expected(inputs, nbytes, klass, np.full(n, 64))
        assert want["result"]["n_flows"] == n and (want["flow_id"] == np.arange(n)).all()
        run(gpu_ctx, abi.Batch(d.ptr, None, 64, n, 0, 0, 0), n, want, where="c1 stride 64")
    finally:
        d.free()


EXTRA = _tcp([203, 0, 113, 77], [198, 51, 100, 9], 1, 2)


def _c3_plus_one(ctx):
    """c3's 4,096 flows and one crafted frame whose key none of them has."""
    g, _ = load_golden("c3")
    extra = EXTRA
    inputs, _, _ = golden_keys("c3")
    assert not (inputs[:, :12] == np.frombuffer(fr.walk(extra)[0], np.uint8)).all(axis=1).any()
    at = (len(g["data"]) + 3) // 4 * 4 + 1
    data = np.concatenate([g["data"], np.zeros(at - len(g["data"]), np.uint8), np.frombuffer(extra, np.uint8)])
    desc = np.concatenate([g["desc"], np.array([at | len(extra) << 48], np.uint64)])
    return Source(ctx, "c3", len(desc), data=data, desc=desc)


def test_a_table_with_exactly_as_many_slots_as_flows(gpu_ctx):
    g, _ = load_golden("c3")
    n = 2 * 4096 + 100   # every flow twice and more
    src = Source(gpu_ctx, "c3", n)
    try:
        want = src.want(slots=4096)
        assert want["result"]["n_flows"] == 4096 == want["result"]["slots"] and want["result"]["overflow_packets"] == 0
        run(gpu_ctx, src.batch, n, want, slots=4096, where="4096 flows in 4096 slots")
    finally:
        src.free()


def test_one_flow_more_than_the_slots_reports_overflow(gpu_ctx):
    src = _c3_plus_one(gpu_ctx)
    try:
        n = src.n
        assert n == 4097
        res = run(gpu_ctx, src.batch, n, None, slots=4096, overflow=True)   # the guards are checked in run()
        assert res["overflow_packets"] != 0 and res["n"] == n and res["slots"] == 4096
        # with room for it, the same batch has 4,097 flows
        inputs, nbytes, klass = golden_keys("c3")
        ei, en, ek = fr.key_of_frames([EXTRA])
        want = ftr.expected(np.concatenate([inputs, ei]), np.concatenate([nbytes, en]), np.concatenate([klass, ek]), src.lens,
                            slots=8192)
        assert want["result"]["n_flows"] == 4097
        run(gpu_ctx, src.batch, n, want, slots=8192, where="4097 flows in 8192 slots")
    finally:
        src.free()


@pytest.mark.parametrize("kind", ["random", "ones", "zeros", "null"])
def test_select(gpu_ctx, kind):
    n = 16384 + 999   # the last word has garbage above n
    src = Source(gpu_ctx, "fuzz", n)
    try:
        sel = select_words(kind, n)
        want = src.want(ftr.BIDIRECTIONAL, sel)
        assert (want["result"]["n_selected"] == 0) == (kind == "zeros")
        run(gpu_ctx, src.batch, n, want, ftr.BIDIRECTIONAL, sel, where=kind)
    finally:
        src.free()


def test_flow_cap_below_the_flows(gpu_ctx):
    n = 8192 + 4321
    src = Source(gpu_ctx, "fuzz", n)
    try:
        nf = src.want()["result"]["n_flows"]
        assert nf == 3541
        for cap in (0, 1, nf - 1, nf):
            want = src.want(flow_cap=cap)
            assert want["result"]["n_written"] == cap and want["result"]["n_flows"] == nf
            run(gpu_ctx, src.batch, n, want, flow_cap=cap, where=f"flow_cap={cap}")
    finally:
        src.free()


def test_bytes_cuts_the_last_frames_key(gpu_ctx):
    """`bytes` ends inside the last frame's key: the missing bytes read as zeros, so the key is
    the restatement's over the zero-padded frame."""
    frames = [_tcp([10, 0, 0, 1], [10, 0, 0, 2], 1000 + k, 80) for k in range(20)]
    src0 = _crafted(gpu_ctx, frames, 20)
    last = int(src0.desc[-1] & fr.MASK48)
    src0.free()
    for cut in (last + 36, last + 32, last + 48, last + 16):   # inside the ports, the addresses; behind them; before the IP header
        padded = [f if k < 19 else f[:cut - last] + bytes(len(f) - (cut - last)) for k, f in enumerate(frames)]
        want = ftr.of_frames(padded)
        src = _crafted(gpu_ctx, frames, 20, nbytes=cut)
        try:
            assert src.d_data.nbytes >= cut
            run(gpu_ctx, src.batch, 20, want, where=f"cut={cut}")
        finally:
            src.free()


def _outputs_equal(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("flow_id", "flows", "result"))


@pytest.mark.parametrize("name", ["c3", "fuzz"])
def test_runs_are_byte_equal_and_equal_the_host(gpu_ctx, manifest, name):
    """The same call twice, once more on a caller's stream right behind bt_parse_filter_device with
    its verdict words as `select`, and bt_flow_table_host over the same batch: identical bytes."""
    g, _ = load_golden(name)
    n = 3 * 16384 + 17
    src = Source(gpu_ctx, name, n)
    passed = np.resize(g["code__c3"] == 0, n)
    sel = fr.pack_bits(passed)
    want = src.want(ftr.BIDIRECTIONAL, sel)
    assert 0 < want["result"]["n_selected"] < n
    gpu_ctx.compile(manifest["filter_sets"]["c3"])
    d_ver, d_dec = gpu_ctx.alloc(8 * ((n + 63) // 64)), gpu_ctx.alloc(n)
    st = gpu_ctx.stream_create()
    try:
        a = run(gpu_ctx, src.batch, n, want, ftr.BIDIRECTIONAL, sel, where="first")
        b = run(gpu_ctx, src.batch, n, want, ftr.BIDIRECTIONAL, sel, where="second")
        gpu_ctx.run_device(src.batch, abi.Outputs(None, 0, d_ver.ptr, d_dec.ptr, None, None), st)
        c = run(gpu_ctx, src.batch, n, want, ftr.BIDIRECTIONAL, sel, stream=st, d_select=d_ver, where="behind the filter")
        assert _outputs_equal(a, b) and _outputs_equal(a, c)
        fid, flows, res = abi.flow_table_host(g["data"], src.desc, abi.FlowTableOpts(ftr.BIDIRECTIONAL, 0, n, 0), sel)
        assert fid.tobytes() == a["flow_id"].tobytes() and flows.tobytes() == a["flows"][:80 * res["n_written"]].tobytes()
        assert res == abi.FlowTableResult.from_bytes(a["result"]).as_dict()
    finally:
        gpu_ctx.stream_destroy(st)
        gpu_ctx.compile([])
        for x in (d_ver, d_dec):
            x.free()
        src.free()


def test_an_empty_batch_still_writes_the_result(gpu_ctx):
    res = Guarded(gpu_ctx, 72)
    st = gpu_ctx.stream_create()
    try:
        gpu_ctx.flow_table_device(abi.Batch(None, None, 64, 0, 0, 0, 0), abi.FlowTableOpts(0, 512, 0, 0), None, 0, res.ptr,
                                  stream=st)
        gpu_ctx.stream_synchronize(st)
        got = abi.FlowTableResult.from_bytes(res.read()).as_dict()
        assert got == ftr.expected(np.zeros((0, 36), np.uint8), np.zeros(0, np.int64), np.zeros(0, np.int64), [], slots=512)["result"]
    finally:
        gpu_ctx.stream_destroy(st)
        res.free()
