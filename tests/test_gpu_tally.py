"""GPU: bt_tally_device (beatrice_amd/csrc/bt_tally.hip), the counts of a device-resident batch.
Expected values come from the numpy restatement below (_reference), never from the code under
test: np.bincount over the decision bytes (cut at the first THROW when stopping), the frame
lengths summed by code over the same range, the present / ok bits of rec[:, 24:26] over [0, n),
and the first THROW / HOST indices. *out sits in a poisoned buffer between two 256-byte guards."""
import ctypes

import numpy as np
import pytest

from beatrice_amd import abi
from conftest import load_golden

pytestmark = pytest.mark.gpu

POISON = 0xC7
GUARD = 256
SIZE = 2304
CHUNK = 16384
BT_E_INVALID_ARGUMENT = 1
STOP, ACC = abi.TALLY_STOP_AT_THROW, abi.TALLY_ACCUMULATE
SIZES = [0, 1, 63, 64, 65, 16383, 16384, 16385, 3 * 16384 + 17]
LENGTHS = np.array([0, 1, 60, 1514, 65535], np.int64)


def _reference(dec=None, lens=None, layers=None, stop=False, n=None):
    """The expected bt_tally as a dict. dec: n decision bytes; lens: n frame lengths; layers:
    [n, 2] present / ok bytes."""
    n = len(dec) if dec is not None else n
    t = {"n": n, "scanned": n, "first_throw": n, "first_host": n, "first_throw_slot": 0, "first_host_slot": 0,
         "code": [0] * 4, "slot": [[0] * 64 for _ in range(4)], "bytes": [0] * 4, "layer_present": [0] * 8,
         "layer_ok": [0] * 8, "reserved": [0] * 3}
    if dec is not None:
        thr, host = np.nonzero(dec >> 6 == 2)[0], np.nonzero(dec >> 6 == 3)[0]
        if len(thr):
            t["first_throw"], t["first_throw_slot"] = int(thr[0]), int(dec[thr[0]] & 63)
        if len(host):
            t["first_host"], t["first_host_slot"] = int(host[0]), int(dec[host[0]] & 63)
        cut = t["first_throw"] if stop else n
        t["scanned"] = cut
        hist = np.bincount(dec[:cut], minlength=256).reshape(4, 64)
        t["slot"] = hist.tolist()
        t["code"] = hist.sum(axis=1).tolist()
        if lens is not None:
            t["bytes"] = [int(lens[:cut][dec[:cut] >> 6 == k].sum()) for k in range(4)]
    if layers is not None:
        t["layer_present"] = [int(((layers[:n, 0] >> k) & 1).sum()) for k in range(8)]
        t["layer_ok"] = [int(((layers[:n, 1] >> k) & 1).sum()) for k in range(8)]
    return t


def _sum(a, b):
    """What BT_TALLY_ACCUMULATE leaves after tally a, then b: sums, with b's first_* fields."""
    t = dict(b)
    for k in ("n", "scanned"):
        t[k] = a[k] + b[k]
    for k in ("code", "bytes", "layer_present", "layer_ok"):
        t[k] = [x + y for x, y in zip(a[k], b[k])]
    t["slot"] = [[x + y for x, y in zip(ra, rb)] for ra, rb in zip(a["slot"], b["slot"])]
    return t


class Out:
    """A bt_tally on the device between two guards, poisoned."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.buf = ctx.alloc(GUARD + SIZE + GUARD)
        self.ptr = self.buf.ptr + GUARD
        self.poison()

    def poison(self):
        abi._check(abi.lib().bt_memset_d(self.ctx.h, self.buf.ptr, POISON, self.buf.nbytes))

    def raw(self):
        self.ctx.synchronize()
        full = self.buf.download(np.zeros(self.buf.nbytes, np.uint8))
        assert (full[:GUARD] == POISON).all() and (full[GUARD + SIZE:] == POISON).all(), "guard bytes written"
        return full[GUARD:GUARD + SIZE]

    def read(self):
        return abi.Tally.from_bytes(self.raw()).as_dict()

    def free(self):
        self.buf.free()


@pytest.fixture()
def out(gpu_ctx):
    o = Out(gpu_ctx)
    yield o
    o.free()


class Decisions:
    """Decision bytes on the device at a byte offset from a 16-byte boundary; every other byte of
    the buffer holds a THROW at slot 63, which a read outside [0, n) would count."""

    def __init__(self, ctx, dec, off=0):
        self.dec = np.ascontiguousarray(dec, np.uint8)
        self.buf = ctx.alloc(len(self.dec) + 64)
        host = np.full(self.buf.nbytes, 0xBF, np.uint8)
        host[off:off + len(self.dec)] = self.dec
        self.buf.upload(host)
        assert self.buf.ptr % 16 == 0
        self.ptr = self.buf.ptr + off

    def free(self):
        self.buf.free()


def _random(n, seed, codes=None):
    rng = np.random.default_rng(seed)
    dec = rng.integers(0, 256, n, dtype=np.uint8)
    if codes is not None:   # only these codes, any slot
        dec = (np.asarray(codes, np.uint8)[rng.integers(0, len(codes), n)] << 6 | (dec & 63)).astype(np.uint8)
    return dec


def _one(ctx, out, dec, flags=0, off=0, where=""):
    d = Decisions(ctx, dec, off)
    try:
        out.poison()
        ctx.tally_device(d.ptr, len(dec), out.ptr, flags=flags)
        got = out.read()
    finally:
        d.free()
    want = _reference(dec, stop=bool(flags & STOP))
    assert got == want, f"{where}: " + ", ".join(k for k in want if got[k] != want[k])
    return got


@pytest.mark.parametrize("n", SIZES)
def test_random_bytes_at_tile_and_chunk_edges(gpu_ctx, out, n):
    """All 256 byte values, decide at pointer offsets 0, 1 and 5 from a 16-byte boundary."""
    dec = _random(n, 100 + n)
    for off in (0, 1, 5):
        for flags in (0, STOP):
            _one(gpu_ctx, out, dec, flags, off, f"n={n} off={off} flags={flags}")


def test_no_throw_at_all(gpu_ctx, out):
    n = SIZES[-1]
    dec = _random(n, 1, codes=[0, 1, 3])
    for flags in (0, STOP):
        t = _one(gpu_ctx, out, dec, flags, 1, f"no throw flags={flags}")
        assert t["first_throw"] == n and t["scanned"] == n and t["code"][2] == 0 and t["first_host"] < n


@pytest.mark.parametrize("at", [0, 63, 64, 16383, 16384, SIZES[-1] - 1])
def test_single_throw(gpu_ctx, out, at):
    n = SIZES[-1]
    dec = _random(n, 2, codes=[0, 1])
    dec[at] = 0x80 | 37
    for flags in (0, STOP):
        t = _one(gpu_ctx, out, dec, flags, 5, f"throw at {at} flags={flags}")
        assert (t["first_throw"], t["first_throw_slot"]) == (at, 37)
        assert t["scanned"] == (at if flags else n) and t["code"][2] == (0 if flags else 1)
        assert sum(t["code"]) == t["scanned"]


def test_several_throws_and_hosts_around_them(gpu_ctx, out):
    """The first THROW decides; HOST decisions before and after it: first_host covers [0, n) and
    HOST never stops the count."""
    n = SIZES[-1]
    dec = _random(n, 3, codes=[0, 1])
    dec[[20000, 20001, 33000, n - 1]] = 0x80 | 2
    dec[[100, 19999]] = 0xC0 | 9           # before the throw
    dec[[20002, 40000]] = 0xC0 | 11        # after it
    for flags in (0, STOP):
        t = _one(gpu_ctx, out, dec, flags, 0, f"several flags={flags}")
        assert (t["first_throw"], t["first_host"], t["first_host_slot"]) == (20000, 100, 9)
        assert t["code"][3] == (2 if flags else 4) and t["slot"][3][9] == 2
    dec[[100, 19999]] = 1                  # the only HOST decisions left lie behind the throw
    for flags in (0, STOP):
        t = _one(gpu_ctx, out, dec, flags, 0, f"host after throw flags={flags}")
        assert (t["first_host"], t["first_host_slot"]) == (20002, 11) and t["code"][3] == (0 if flags else 2)


def _frames(ctx, form, n):
    """(Batch, lengths, buffers) for one frame form over n packets; the frames' bytes are never read."""
    lens = LENGTHS[np.arange(n) % len(LENGTHS)]
    rng = np.random.default_rng(n)
    lens = lens[rng.permutation(n)] if n else lens
    bufs = []
    if form in ("packed", "xdp"):
        base = ctx.alloc(65536 + 256)
        bufs.append(base)
        if form == "packed":
            raw = (lens.astype(np.uint64) << np.uint64(48))
        else:
            raw = np.zeros(n, np.dtype([("addr", "<u8"), ("len", "<u4"), ("options", "<u4")]))
            raw["len"], raw["options"] = lens, rng.integers(0, 1 << 32, n, dtype=np.uint32)
        d = ctx.alloc(max(16, raw.nbytes))
        d.upload(raw)
        bufs.append(d)
        return abi.Batch(base.ptr, d.ptr, 0, n, 65536, abi.DESC_XDP if form == "xdp" else abi.DESC_PACKED, 0), lens, bufs
    stride = int(form)
    base = ctx.alloc(max(16, n * stride))
    bufs.append(base)
    return abi.Batch(base.ptr, None, stride, n, n * stride, 0, 0), np.full(n, min(stride, 65535), np.int64), bufs


@pytest.mark.parametrize("form,n", [("packed", SIZES[-1]), ("xdp", SIZES[-1]), ("64", 16385), ("200", 16385),
                                    ("packed", 65), ("xdp", 1)])
def test_byte_sums_over_the_frame_forms(gpu_ctx, out, form, n):
    batch, lens, bufs = _frames(gpu_ctx, form, n)
    dec = _random(n, 7, codes=[0, 1, 3])
    thrown = dec.copy()
    thrown[n // 2] = 0x80
    try:
        for d_host, flags in ((dec, 0), (dec, STOP), (thrown, 0), (thrown, STOP)):
            d = Decisions(gpu_ctx, d_host, 1)
            out.poison()
            gpu_ctx.tally_device(d.ptr, n, out.ptr, frames=batch, flags=flags)
            got = out.read()
            d.free()
            want = _reference(d_host, lens, stop=bool(flags & STOP))
            assert got == want, f"{form} n={n} flags={flags}"
            assert sum(got["bytes"]) == int(lens[:got["scanned"]].sum())
        d = Decisions(gpu_ctx, dec)
        out.poison()
        gpu_ctx.tally_device(d.ptr, n, out.ptr)   # frames = NULL: zeros
        assert out.read()["bytes"] == [0, 0, 0, 0]
        d.free()
    finally:
        for b in bufs:
            b.free()


LAYOUTS = {"tiled": 0, "planes": abi.OPT_RECORDS_PLANES, "aos": abi.OPT_RECORDS_AOS}


@pytest.fixture(scope="module", params=list(LAYOUTS))
def layout_ctx(request):
    ctx = abi.Context(0, flags=LAYOUTS[request.param])
    yield request.param, ctx
    ctx.close()


def _device_records(layout, rec):
    """The golden records in a device layout; every byte no record of [0, n) owns is random,
    the tail slots of the last tile included."""
    n = len(rec)
    rng = np.random.default_rng(n)
    if layout == "aos":
        return np.concatenate([rec.reshape(-1), rng.integers(0, 256, 64 * 96, dtype=np.uint8)])
    c, ns = abi.pack_records(rec), abi.record_slabs(rec)
    if layout == "planes":
        return abi.tile_packed(c, ns, planes=True)
    t = abi.tile_packed(c, ns).reshape(-1, 6, 64, 16)
    if n % 64:
        t[-1, 0:2, n % 64:] = rng.integers(0, 256, (2, 64 - n % 64, 16), dtype=np.uint8)
    return t.reshape(-1)


@pytest.mark.parametrize("cap", ["edge", "fuzz"])
def test_layer_counts_in_every_record_layout(layout_ctx, cap):
    layout, ctx = layout_ctx
    g, _ = load_golden(cap)
    rec = g["rec"]
    n_all = len(rec)
    assert n_all == {"edge": 319, "fuzz": 8192}[cap]
    image = _device_records(layout, rec)
    d_rec = ctx.alloc(len(image))
    d_rec.upload(image)
    out = Out(ctx)
    dec = _random(n_all, 5, codes=[0, 1, 3])
    d = Decisions(ctx, dec)
    try:
        for n in (n_all, 100):   # 100: a partial last tile whose other lanes hold real records
            out.poison()
            ctx.tally_device(None, n, out.ptr, records_ptr=d_rec, n_cap=n_all)   # decide = NULL: layers only
            got = out.read()
            want = _reference(None, None, rec[:, 24:26], n=n)
            assert got == want, f"{layout} {cap} n={n} layers only"
            assert sum(got["layer_present"]) > 0 and sum(got["code"]) == 0
            out.poison()
            ctx.tally_device(d.ptr, n, out.ptr, records_ptr=d_rec, n_cap=n_all, flags=STOP)
            assert out.read() == _reference(dec[:n], None, rec[:, 24:26], stop=True), f"{layout} {cap} n={n}"
    finally:
        for b in (d_rec, out, d):
            b.free()


def test_accumulate(gpu_ctx, out):
    a, b = _random(20000, 11, codes=[0, 1, 3]), _random(777, 12, codes=[0, 1, 3])
    b[500] = 0x80 | 4
    fa, la, bufs_a = _frames(gpu_ctx, "packed", len(a))
    fb, lb, bufs_b = _frames(gpu_ctx, "xdp", len(b))
    da, db = Decisions(gpu_ctx, a, 1), Decisions(gpu_ctx, b, 5)
    try:
        gpu_ctx.tally_device(da.ptr, len(a), out.ptr, frames=fa, flags=STOP)
        gpu_ctx.tally_device(db.ptr, len(b), out.ptr, frames=fb, flags=STOP | ACC)
        want = _sum(_reference(a, la, stop=True), _reference(b, lb, stop=True))
        assert out.read() == want
        assert want["first_throw"] == 500 and want["n"] == 20777 and want["scanned"] == 20500
        for _ in range(2):   # the 64-bit adds go on
            gpu_ctx.tally_device(db.ptr, len(b), out.ptr, frames=fb, flags=STOP | ACC)
            want = _sum(want, _reference(b, lb, stop=True))
        assert out.read() == want and want["n"] == 20000 + 3 * 777
        # an empty batch: nothing to add, the first_* fields are this call's
        gpu_ctx.tally_device(db.ptr, 0, out.ptr, flags=ACC)
        assert out.read() == _sum(want, _reference(b[:0]))
    finally:
        for x in (da, db, *bufs_a, *bufs_b):
            x.free()


def test_refusals_leave_out_untouched(gpu_ctx, out):
    L = abi.lib()
    dec = Decisions(gpu_ctx, _random(319, 1))
    batch, _, bufs = _frames(gpu_ctx, "packed", 319)
    rec = gpu_ctx.alloc(5 * 6144)

    def call(ctx=gpu_ctx.h, decide=dec.ptr, n=319, frames=None, records=None, n_cap=0, flags=0, o=out.ptr):
        return L.bt_tally_device(ctx, decide, n, ctypes.byref(frames) if frames is not None else None, records, n_cap,
                                 flags, o, None)
    try:
        assert call(ctx=None) == BT_E_INVALID_ARGUMENT
        assert call(o=None) == BT_E_INVALID_ARGUMENT
        assert call(o=out.ptr + 4) == BT_E_INVALID_ARGUMENT                 # not 8-byte aligned
        assert call(decide=None) == BT_E_INVALID_ARGUMENT                   # decide and records both NULL
        assert call(frames=batch, n=318) == BT_E_INVALID_ARGUMENT           # frames->n != n
        nb = abi.Batch(batch.base, batch.desc, 0, 319, 0, 0, 0)
        assert call(frames=nb) == BT_E_INVALID_ARGUMENT                     # a descriptor batch must state its size
        nb = abi.Batch(batch.base, batch.desc, 0, 319, 65536, 2, 0)
        assert call(frames=nb) == BT_E_INVALID_ARGUMENT                     # unknown desc_format
        nb = abi.Batch(None, batch.desc, 0, 319, 65536, 0, 0)
        assert call(frames=nb) == BT_E_INVALID_ARGUMENT                     # null packet buffer
        nb = abi.Batch(batch.base, None, 0, 319, 0, 0, 0)
        assert call(frames=nb) == BT_E_INVALID_ARGUMENT                     # fixed stride 0
        assert call(records=rec.ptr, n_cap=318) == BT_E_INVALID_ARGUMENT    # n_cap < n
        for flags in (0x4, 0x80000000, 0x7):
            assert call(flags=flags) == BT_E_INVALID_ARGUMENT, flags
        assert (out.raw() == POISON).all()
        assert call(frames=batch, records=rec.ptr, n_cap=319, flags=STOP | ACC) == 0   # and the full form is taken
        gpu_ctx.synchronize()
    finally:
        for b in (dec, rec, *bufs):
            b.free()


def test_empty_batch_writes_out(gpu_ctx, out):
    d = gpu_ctx.alloc(64)
    gpu_ctx.tally_device(d.ptr, 0, out.ptr)
    assert not out.raw().any()
    d.free()


E2E_SETS = ["c3", "mixed", "throw_after", "port_range_5", "payload_mid", "empty"]


@pytest.mark.parametrize("cap", ["fuzz", "edge"])
def test_behind_parse_filter_on_one_stream(gpu_ctx, out, manifest, cap):
    """bt_parse_filter_device, then bt_tally_device on the same stream with no wait in between."""
    g, _ = load_golden(cap)
    n = len(g["desc"])
    lens = (g["desc"] >> np.uint64(48)).astype(np.int64)
    run = abi.DeviceRun(gpu_ctx, g["data"], g["desc"], n)
    try:
        for fset in E2E_SETS:
            gpu_ctx.compile(manifest["filter_sets"][fset])
            for flags in (0, STOP):
                out.poison()
                run.run()
                gpu_ctx.tally_device(run.d_dec, n, out.ptr, frames=run.batch, records_ptr=run.d_rec, n_cap=n,
                                     flags=flags)
                got = out.read()
                res = run.fetch()
                want = _reference(res["decide"], lens, g["rec"][:, 24:26], stop=bool(flags))
                assert got == want, f"{cap}/{fset} flags={flags}"
                if not flags:
                    assert got["code"][abi.DECIDE_PASS] == res["n_pass"]
                if (cap, fset) == ("fuzz", "throw_after"):
                    assert got["first_throw"] == 8 and got["scanned"] == (8 if flags else n)
    finally:
        run.free()
