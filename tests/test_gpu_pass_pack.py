"""GPU: bt_pass_pack_device (beatrice_amd/csrc/bt_pack.hip), the ordered pack of the selected
frames of a device-resident batch. Expected bytes, descriptors, total and n_packed come from the
numpy restatement below (_reference), never from the code under test: record k = `lead` bytes
in front of the k-th selected frame + min(len, snap or len) frame bytes (source bytes outside
the buffer are zeros), placed at the sum of the earlier slots (record size rounded up to
`align`, gap bytes zero); a slot is written only when it ends at or below cap."""
import ctypes

import numpy as np
import pytest

from beatrice_amd import abi
from conftest import load_golden

pytestmark = pytest.mark.gpu

POISON = 0xC7
GUARD = 256
MASK48 = np.uint64((1 << 48) - 1)
BT_E_INVALID_ARGUMENT = 1


def _words(sel: np.ndarray, garbage=False) -> np.ndarray:
    """Verdict-layout words of a bool selection; garbage: the bits at or above n set."""
    n = len(sel)
    bits = np.zeros((n + 63) // 64 * 64, np.uint8)
    bits[:n] = sel
    if garbage:
        bits[n:] = 1
    return np.packbits(bits, bitorder="little").view(np.uint64) if len(bits) else np.zeros(1, np.uint64)


def _source(data: np.ndarray, nbytes: int, lo: int, hi: int) -> np.ndarray:
    """Bytes [lo, hi) of the source buffer, zeros outside [0, nbytes)."""
    out = np.zeros(hi - lo, np.uint8)
    a, b = max(lo, 0), min(hi, nbytes)
    if b > a:
        out[a - lo:b - lo] = data[a:b]
    return out


def _reference(data, nbytes, off, ln, sel, lead, snap, align, cap):
    """(bytes written [0, limit), descriptors of every selected packet, total, n_packed)."""
    idx = np.nonzero(sel)[0]
    cl = ln[idx].astype(np.int64)
    if snap:
        cl = np.minimum(cl, snap)
    slot = (lead + cl + align - 1) // align * align
    start = np.cumsum(slot) - slot
    total = int(slot.sum())
    n_packed = int(((start + slot) <= cap).sum())
    assert not n_packed or bool(((start + slot)[:n_packed] <= cap).all())   # a prefix
    limit = int((start + slot)[n_packed - 1]) if n_packed else 0
    out = np.zeros(limit, np.uint8)
    for k in range(n_packed):
        o = int(off[idx[k]])
        out[start[k]:start[k] + lead + cl[k]] = _source(data, nbytes, o - lead, o + int(cl[k]))
    desc = (start + lead).astype(np.uint64) | (cl.astype(np.uint64) << np.uint64(48))
    return out, desc, total, n_packed


class Source:
    """A batch's frames (and descriptors) on the device, shared by the runs of one test."""

    def __init__(self, ctx, data, desc=None, stride=0, n=None, nbytes=None, desc_format=abi.DESC_PACKED):
        self.ctx = ctx
        self.data = np.ascontiguousarray(data, np.uint8)
        self.nbytes = len(self.data) if nbytes is None else nbytes
        self.d_data = ctx.alloc(len(self.data) + 256)
        self.d_data.upload(self.data)
        self.d_desc = None
        self.stride = stride
        if desc is not None:
            self.n = len(desc) if n is None else n
            self.off = (desc & MASK48).astype(np.int64)
            self.len = (desc >> np.uint64(48)).astype(np.int64)
            raw = desc
            if desc_format == abi.DESC_XDP:   # struct xdp_desc {u64 addr; u32 len; u32 options}
                raw = np.zeros(len(desc), np.dtype([("addr", "<u8"), ("len", "<u4"), ("options", "<u4")]))
                raw["addr"], raw["len"], raw["options"] = self.off, self.len, 0xFEEDBEEF
            self.d_desc = ctx.alloc(max(16, raw.nbytes))
            self.d_desc.upload(raw)
        else:
            self.n = n
            self.off = np.arange(n, dtype=np.int64) * stride
            self.len = np.full(n, min(stride, 65535), np.int64)
        self.desc_format = desc_format

    def batch(self, n=None, flags=0):
        return abi.Batch(self.d_data.ptr, self.d_desc.ptr if self.d_desc else None, self.stride,
                         self.n if n is None else n, self.nbytes, self.desc_format, flags)

    def free(self):
        self.d_data.free()
        if self.d_desc:
            self.d_desc.free()


def _pack(src, sel, lead=0, snap=0, align=1, cap=None, room=None, shift=0, garbage=False, n=None):
    """One bt_pass_pack_device call into a poisoned buffer with guards. Returns (the `room`
    bytes from the output pointer on, descriptors, total, n_packed, front guard, back guard)."""
    ctx = src.ctx
    n = src.n if n is None else n
    sel = np.asarray(sel, bool)[:n]
    words = _words(sel, garbage)
    if room is None:
        room = int((lead + src.len[:n][sel] + 63).sum()) + 64
    if cap is None:
        cap = room
    assert cap <= room
    size = GUARD + shift + room + GUARD
    d_out, d_sel = ctx.alloc(size), ctx.alloc(max(16, words.nbytes))
    d_odesc, d_tot = ctx.alloc(max(16, n * 8)), ctx.alloc(16)
    try:
        for b in (d_out, d_odesc, d_tot):
            abi._check(abi.lib().bt_memset_d(ctx.h, b.ptr, POISON, b.nbytes))
        d_sel.upload(words)
        ctx.pass_pack(src.batch(n), d_sel, d_out.ptr + GUARD + shift, cap, d_tot.ptr, d_tot.ptr + 8, desc=d_odesc,
                      lead=lead, snap=snap, align=align)
        ctx.synchronize()
        full = d_out.download(np.zeros(size, np.uint8))
        odesc = d_odesc.download(np.zeros(max(2, n), np.uint64))[:n]
        tot = d_tot.download(np.zeros(16, np.uint8))
    finally:
        for b in (d_out, d_sel, d_odesc, d_tot):
            b.free()
    body = full[GUARD + shift:GUARD + shift + room]
    return (body, odesc, int(tot[:8].view(np.uint64)[0]), int(tot[8:12].view(np.uint32)[0]),
            full[:GUARD + shift], full[GUARD + shift + room:])


def _check(src, sel, lead=0, snap=0, align=1, cap=None, room=None, shift=0, garbage=False, n=None, where=""):
    n_ = src.n if n is None else n
    sel = np.asarray(sel, bool)[:n_]
    body, odesc, total, n_packed, g0, g1 = _pack(src, sel, lead, snap, align, cap, room, shift, garbage, n)
    cap_ = len(body) if cap is None else cap
    want, wdesc, wtotal, wpacked = _reference(src.data, src.nbytes, src.off[:n_], src.len[:n_], sel, lead, snap,
                                              align, cap_)
    assert total == wtotal, f"{where}: total {total} != {wtotal}"
    assert n_packed == wpacked, f"{where}: n_packed {n_packed} != {wpacked}"
    assert (g0 == POISON).all() and (g1 == POISON).all(), f"{where}: guard bytes written"
    assert len(want) <= cap_
    bad = np.nonzero(body[:len(want)] != want)[0]
    assert len(bad) == 0, f"{where}: {len(bad)} packed bytes differ, first at {bad[:5]}"
    assert (body[len(want):] == POISON).all(), f"{where}: bytes written past the last fitting record"
    k = int(sel.sum())
    assert np.array_equal(odesc[:k], wdesc), f"{where}: descriptors differ"
    assert (odesc[k:] == np.uint64(0xC7C7C7C7C7C7C7C7)).all(), f"{where}: descriptors past the selection written"
    return total, n_packed


GOLDEN_CASES = [("c3", "c3", 356, 4096), ("c3", "custom", 3765, 4096), ("c4", "mixed", 11, 2048),
                ("edge", "mixed", 100, 319), ("edge", "bpf_3", 7, 319), ("http", "payload_re_11", 2476, 3000),
                ("edge", "empty", 319, 319), ("c3", "empty", 4096, 4096), ("edge", "bpf_7", 0, 319)]


@pytest.mark.parametrize("cap,fset,n_sel,n", GOLDEN_CASES)
def test_goldens(gpu_ctx, cap, fset, n_sel, n):
    g, _ = load_golden(cap)
    sel = g[f"code__{fset}"] == 0
    assert len(sel) == n and int(sel.sum()) == n_sel   # the selection is what the issue states
    src = Source(gpu_ctx, g["data"], g["desc"])
    try:
        for lead, snap, align, shift in [(0, 0, 1, 0), (16, 0, 1, 5), (16, 0, 64, 0), (3, 96, 16, 8)]:
            total, packed = _check(src, sel, lead, snap, align, shift=shift, where=f"{cap}/{fset} {lead}/{snap}/{align}")
            assert packed == n_sel
    finally:
        src.free()


def test_goldens_xdp_descriptors(gpu_ctx):
    g, _ = load_golden("edge")
    sel = g["code__mixed"] == 0
    assert int(sel.sum()) == 100
    src = Source(gpu_ctx, g["data"], g["desc"], desc_format=abi.DESC_XDP)
    try:
        _check(src, sel, 16, 0, 1, where="edge/mixed xdp")
        _check(src, sel, 0, 60, 16, where="edge/mixed xdp snap")
    finally:
        src.free()


SWEEP_LENGTHS = [0, 1, 15, 16, 17, 31, 33, 63, 64, 65, 1500, 65535]


@pytest.fixture(scope="module")
def sweep(gpu_ctx):
    """Every length at every source residue 0..15 mod 16 (odd ones included), random bytes."""
    rng = np.random.default_rng(7)
    desc, pos = [], 0
    for res in range(16):
        for ln in SWEEP_LENGTHS:
            pos += (res - pos) % 16 or 16   # at least one byte of other data between frames
            desc.append(pos | (ln << 48))
            pos += ln
    data = rng.integers(0, 256, pos + 40, dtype=np.uint8)
    src = Source(gpu_ctx, data, np.array(desc, np.uint64))
    assert sorted(set((src.off % 16).tolist())) == list(range(16)) and src.n == 192
    yield src
    src.free()


@pytest.mark.parametrize("snap", [0, 60])
@pytest.mark.parametrize("align", [1, 16, 64])
@pytest.mark.parametrize("lead", [0, 16])
def test_alignment_sweep(sweep, lead, align, snap):
    sel = np.ones(sweep.n, bool)
    sel[4::7] = False   # dropped frames shift the records behind them: destination residues vary
    _check(sweep, sel, lead, snap, align, shift=(lead + align + snap) % 16, where=f"sweep {lead}/{align}/{snap}")
    if align == 1:      # at align 1 every destination residue occurs
        cl = np.minimum(sweep.len[sel], snap) if snap else sweep.len[sel]
        starts = np.cumsum(lead + cl) - (lead + cl)
        assert len(set((starts % 16).tolist())) == 16


SEAM_N = [1, 63, 64, 65, 16383, 16384, 16385, 33000]


@pytest.fixture(scope="module")
def fixed64(gpu_ctx):
    rng = np.random.default_rng(11)
    src = Source(gpu_ctx, rng.integers(0, 256, 33000 * 64, dtype=np.uint8), stride=64, n=33000)
    yield src
    src.free()


@pytest.mark.parametrize("n", SEAM_N)
def test_scan_seams(fixed64, n):
    """64-B fixed-stride frames around the tile (64) and chunk (16,384) boundaries of the scan;
    the expected output of a fixed-size selection is a plain row gather."""
    rows = fixed64.data[:n * 64].reshape(n, 64)
    picks = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "first": np.arange(n) == 0,
             "last": np.arange(n) == n - 1, "every65th": np.arange(n) % 65 == 0}
    for name, sel in picks.items():
        body, odesc, total, n_packed, g0, g1 = _pack(fixed64, sel, n=n, garbage=True, room=n * 64 + 64,
                                                     cap=n * 64 + 64)
        k = int(sel.sum())
        assert (total, n_packed) == (k * 64, k), f"n={n} {name}"
        assert np.array_equal(body[:k * 64], rows[sel].reshape(-1)), f"n={n} {name}"
        assert (body[k * 64:] == POISON).all() and (g0 == POISON).all() and (g1 == POISON).all(), f"n={n} {name}"
        assert np.array_equal(odesc[:k], (np.arange(k, dtype=np.uint64) * np.uint64(64)) | (np.uint64(64) << np.uint64(48)))
    # the general reference agrees with the row gather (one case, with a lead crossing frames)
    _check(fixed64, picks["every65th"], lead=16, align=16, n=n, garbage=True, where=f"n={n} lead")


def test_capacity(gpu_ctx):
    g, _ = load_golden("edge")
    sel = g["code__mixed"] == 0
    src = Source(gpu_ctx, g["data"], g["desc"])
    try:
        total, packed = _check(src, sel, 16, 0, 16, where="roomy")
        assert packed == 100
        room = total + 64
        for cap, n_fit in [(total, 100), (total - 1, 99), (0, None), (total // 2, None)]:
            t, p = _check(src, sel, 16, 0, 16, cap=cap, room=room, shift=1, where=f"cap {cap}")
            assert t == total
            if n_fit is not None:
                assert p == n_fit
            if cap == 0:
                assert p == 0
        # cap 0 as the size query: no output buffer at all
        words = _words(sel)
        d_sel, d_tot = gpu_ctx.alloc(words.nbytes), gpu_ctx.alloc(16)
        d_sel.upload(words)
        gpu_ctx.pass_pack(src.batch(), d_sel, None, 0, d_tot.ptr, d_tot.ptr + 8, lead=16, align=16)
        gpu_ctx.synchronize()
        tot = d_tot.download(np.zeros(16, np.uint8))
        assert int(tot[:8].view(np.uint64)[0]) == total and int(tot[8:12].view(np.uint32)[0]) == 0
        d_sel.free()
        d_tot.free()
    finally:
        src.free()


def test_source_bounds(gpu_ctx):
    """A lead in front of the buffer, descriptors running past it, wholly past it and far past it
    all copy zeros for the bytes the buffer does not hold; `bytes` smaller than the allocation
    is the limit (the bytes behind it are not zero on the device)."""
    rng = np.random.default_rng(3)
    data = rng.integers(1, 256, 4096, dtype=np.uint8)   # no zero byte: a zero in the output was not read
    nbytes = 4000
    desc = np.array([4 | (100 << 48), 200 | (64 << 48), 3990 | (300 << 48), 3999 | (1 << 48), 4000 | (40 << 48),
                     5000 | (50 << 48), (1 << 40) | (33 << 48), ((1 << 48) - 1) | (65535 << 48), 0 | (0 << 48)],
                    np.uint64)
    src = Source(gpu_ctx, data, desc, nbytes=nbytes)
    try:
        sel = np.ones(len(desc), bool)
        for lead, align in [(16, 1), (64, 16), (0, 1), (7, 64)]:
            _check(src, sel, lead, 0, align, shift=3, where=f"bounds {lead}/{align}")
        body, _, _, _, _, _ = _pack(src, sel, lead=16)
        assert not body[:12].any() and body[12] == data[0]       # 12 bytes in front of the buffer, then byte 0
    finally:
        src.free()


def test_offsets_past_32_bits(gpu_ctx):
    """65,600 descriptors over one 65,535-B region: 4.3 GB of output. Every descriptor, total and
    n_packed are checked; of the bytes only the last MiB is downloaded."""
    n, ln = 65600, 65535
    total = n * ln
    assert total > 1 << 32
    rng = np.random.default_rng(5)
    data = rng.integers(0, 256, ln + 64, dtype=np.uint8)
    desc = np.full(n, 1 | (ln << 48), np.uint64)   # an odd source offset
    try:
        d_out = gpu_ctx.alloc(total + GUARD)
    except abi.BtError as e:
        pytest.skip(f"the device has under 6 GiB free: a {total + GUARD}-byte output could not be allocated ({e})")
    src = Source(gpu_ctx, data, desc)
    words = _words(np.ones(n, bool))
    d_sel, d_odesc, d_tot = gpu_ctx.alloc(words.nbytes), gpu_ctx.alloc(n * 8), gpu_ctx.alloc(16)
    try:
        d_sel.upload(words)
        abi._check(abi.lib().bt_memset_d(gpu_ctx.h, d_out.ptr + total, POISON, GUARD))
        gpu_ctx.pass_pack(src.batch(), d_sel, d_out, total, d_tot.ptr, d_tot.ptr + 8, desc=d_odesc)
        gpu_ctx.synchronize()
        tot = d_tot.download(np.zeros(16, np.uint8))
        assert int(tot[:8].view(np.uint64)[0]) == total and int(tot[8:12].view(np.uint32)[0]) == n
        odesc = d_odesc.download(np.zeros(n, np.uint64))
        assert np.array_equal(odesc, (np.arange(n, dtype=np.uint64) * np.uint64(ln)) | (np.uint64(ln) << np.uint64(48)))
        tail = np.zeros((1 << 20) + GUARD, np.uint8)
        abi._check(abi.lib().bt_memcpy_d2h(gpu_ctx.h, tail.ctypes.data, d_out.ptr + total - (1 << 20), tail.nbytes))
        pos = np.arange(total - (1 << 20), total, dtype=np.int64)
        assert np.array_equal(tail[:1 << 20], data[1 + pos % ln])
        assert (tail[1 << 20:] == POISON).all()
        # ... and the bytes around the 2^32 boundary
        mid = np.zeros(4096, np.uint8)
        abi._check(abi.lib().bt_memcpy_d2h(gpu_ctx.h, mid.ctypes.data, d_out.ptr + (1 << 32) - 2048, mid.nbytes))
        pos = np.arange((1 << 32) - 2048, (1 << 32) + 2048, dtype=np.int64)
        assert np.array_equal(mid, data[1 + pos % ln])
    finally:
        for b in (d_out, d_sel, d_odesc, d_tot):
            b.free()
        src.free()


def test_refusals(gpu_ctx):
    g, _ = load_golden("edge")
    src = Source(gpu_ctx, g["data"], g["desc"])
    d = gpu_ctx.alloc(4096)
    L = abi.lib()
    try:
        def call(ctx=gpu_ctx.h, batch=None, select=d.ptr, opts=None, out=None, null_opts=False, null_out=False):
            b = batch if batch is not None else src.batch()
            po = opts if opts is not None else abi.PackOpts(0, 0, 1, 0)
            o = out if out is not None else abi.PackOut(d.ptr + 1024, 1024, None, d.ptr + 2048, d.ptr + 2056)
            return L.bt_pass_pack_device(ctx, ctypes.byref(b) if batch is not False else None, select,
                                         None if null_opts else ctypes.byref(po), None if null_out else ctypes.byref(o),
                                         None)
        abi._check(L.bt_memset_d(gpu_ctx.h, d.ptr, 0, 4096))   # an empty selection
        assert call() == 0
        assert call(ctx=None) == BT_E_INVALID_ARGUMENT
        assert call(batch=False) == BT_E_INVALID_ARGUMENT
        assert call(select=None) == BT_E_INVALID_ARGUMENT
        assert call(null_opts=True) == BT_E_INVALID_ARGUMENT
        assert call(null_out=True) == BT_E_INVALID_ARGUMENT
        assert call(out=abi.PackOut(d.ptr, 64, None, None, d.ptr + 2056)) == BT_E_INVALID_ARGUMENT
        assert call(out=abi.PackOut(d.ptr, 64, None, d.ptr + 2048, None)) == BT_E_INVALID_ARGUMENT
        assert call(out=abi.PackOut(None, 64, None, d.ptr + 2048, d.ptr + 2056)) == BT_E_INVALID_ARGUMENT
        assert call(opts=abi.PackOpts(65, 0, 1, 0)) == BT_E_INVALID_ARGUMENT
        assert call(opts=abi.PackOpts(64, 0, 1, 0)) == 0
        for align in (0, 2, 8, 32, 128):
            assert call(opts=abi.PackOpts(0, 0, align, 0)) == BT_E_INVALID_ARGUMENT, align
        for flags in (abi.BATCH_PREFIXES, abi.BATCH_PREFIXES | abi.BATCH_LEAN, abi.BATCH_LEAN):
            assert call(batch=src.batch(flags=flags)) == BT_E_INVALID_ARGUMENT
        nb = src.batch()
        nb.bytes = 0
        assert call(batch=nb) == BT_E_INVALID_ARGUMENT   # a descriptor batch must state its size
        gpu_ctx.synchronize()
    finally:
        d.free()
        src.free()


def test_second_launch_reuses_the_workspace(gpu_ctx, fixed64):
    """A smaller batch after a larger one (the workspace keeps the larger one's sums), and an
    empty batch: its totals are cleared."""
    sel = np.arange(33000) % 3 == 0
    _check(fixed64, sel, lead=0, align=1, where="large")
    _check(fixed64, sel, lead=0, align=16, n=100, where="small after large")
    _check(fixed64, sel, lead=16, align=1, n=16385, where="two chunks after three")
    d_tot = gpu_ctx.alloc(16)
    abi._check(abi.lib().bt_memset_d(gpu_ctx.h, d_tot.ptr, POISON, 16))
    gpu_ctx.pass_pack(fixed64.batch(0), d_tot, None, 0, d_tot.ptr, d_tot.ptr + 8)
    gpu_ctx.synchronize()
    tot = d_tot.download(np.zeros(16, np.uint8))
    assert not tot[:12].any() and (tot[12:] == POISON).all()
    d_tot.free()
