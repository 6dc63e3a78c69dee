"""GPU: bt_flow_fanout_device (beatrice_amd/csrc/bt_fanout.hip), the selected packets of a
device-resident batch fanned out to K queues by RSS flow hash. Expected values come from the
restatement in flow_ref.py (a bit-serial Toeplitz, the flow-key rule applied to the goldens'
reference-made bt_rec, a Python layer walk for crafted frames), never from the code under test.
Every output sits in a poisoned buffer between two 256-byte guards.

Run as a program (python tests/test_gpu_fanout.py) it checks the contents of three goldens once: the
A/B test starts it in a child process with the Toeplitz knob set the other way."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flow_ref as fr  # noqa: E402
from beatrice_amd import abi  # noqa: E402
from conftest import load_golden  # noqa: E402

pytestmark = pytest.mark.gpu

POISON = 0xC7
GUARD = 256
SIZES = [0, 1, 63, 64, 65, 16383, 16384, 16385, 3 * 16384 + 17]
USER_KEY = bytes((37 * i + 11) & 255 for i in range(40))
KEYS = {"default": (0, None, fr.DEFAULT_KEY), "symmetric": (abi.FANOUT_KEY_SYMMETRIC, None, fr.SYMMETRIC_KEY),
        "user": (0, USER_KEY, USER_KEY)}
OUTPUTS = ("hash", "queue", "idx", "select_q")


class Guarded:
    """`size` bytes on the device between two guards, all poisoned."""

    def __init__(self, ctx, size):
        self.ctx, self.size = ctx, size
        self.buf = ctx.alloc(GUARD + (size + 7) // 8 * 8 + GUARD)
        self.ptr = self.buf.ptr + GUARD
        abi._check(abi.lib().bt_memset_d(ctx.h, self.buf.ptr, POISON, self.buf.nbytes))

    def read(self, dtype=np.uint8):
        full = self.buf.download(np.zeros(self.buf.nbytes, np.uint8))
        assert (full[:GUARD] == POISON).all() and (full[GUARD + self.size:] == POISON).all(), "guard bytes written"
        return full[GUARD:GUARD + self.size].copy().view(dtype)

    def free(self):
        self.buf.free()


class Source:
    """A golden's frame bytes and n descriptors (the golden's, repeated) on the device."""

    def __init__(self, ctx, name, n, xdp=False, data=None, desc=None, nbytes=None):
        g, _ = load_golden(name)
        data = g["data"] if data is None else data
        base = g["desc"] if desc is None else desc
        self.n = n
        self.desc = np.resize(base, n).astype(np.uint64) if n else np.zeros(0, np.uint64)
        self.reps = np.resize(np.arange(len(base)), n) if n else np.zeros(0, np.int64)
        self.lens = (self.desc >> np.uint64(48)).astype(np.int64)
        self.d_data = ctx.alloc(len(data) + 256)
        self.d_data.zero()
        self.d_data.upload(data)
        up = self.desc
        if xdp:   # struct xdp_desc {u64 addr; u32 len; u32 options}
            x = np.zeros((max(n, 1), 2), np.uint64)
            x[:n, 0] = self.desc & fr.MASK48
            x[:n, 1] = self.desc >> np.uint64(48) | np.uint64(0xABCD0000 << 32)
            up = x.reshape(-1)
        self.d_desc = ctx.alloc(max(16, up.nbytes))
        if up.nbytes:
            self.d_desc.upload(up)
        self.batch = abi.Batch(self.d_data.ptr, self.d_desc.ptr, 0, n, len(data) if nbytes is None else nbytes,
                               abi.DESC_XDP if xdp else abi.DESC_PACKED, 0)

    def free(self):
        self.d_data.free()
        self.d_desc.free()


@functools.lru_cache(maxsize=None)
def golden_keys(name, key, l3_only=False):
    """(hash, class) of every packet of a golden from its rec, computed once per key."""
    g, _ = load_golden(name)
    inputs, nbytes, klass = fr.key_of_rec(g["rec"], l3_only)
    return fr.toeplitz_many(key, inputs, nbytes), klass


def make_opts(queues, key="default", reta=None, l3_only=False):
    flags, user, _ = KEYS[key]
    return abi.FanoutOpts.make(queues, flags | (abi.FANOUT_L3_ONLY if l3_only else 0), key=user, reta=reta)


def select_words(kind, n, verdict=None, seed=0):
    """Verdict-layout words of a selection, with garbage in the last word's bits at or above n."""
    ntiles = (n + 63) // 64
    if kind == "null" or ntiles == 0:
        return None
    rng = np.random.default_rng(seed + n)
    if kind == "ones":
        w = np.full(ntiles, ~np.uint64(0))
    elif kind == "zeros":
        w = np.zeros(ntiles, np.uint64)
    elif kind == "random":
        w = rng.integers(0, 1 << 63, ntiles, dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, ntiles, dtype=np.uint64)
    else:
        w = fr.pack_bits(verdict)
    if n % 64:
        w = w.copy()
        w[-1] |= ~np.uint64(0) << np.uint64(n % 64)   # must be ignored
    return w


def run(ctx, batch, n, opts, want, select=None, outputs=OUTPUTS, stream=None, where=""):
    """One call into poisoned, guarded buffers; every requested output and *result against `want`.
    Returns the outputs read back."""
    queues = opts.queues
    ntiles = (n + 63) // 64
    sizes = {"hash": 4 * n, "queue": n, "idx": 4 * n, "select_q": 8 * queues * ntiles}
    bufs = {k: Guarded(ctx, sizes[k]) for k in outputs}
    res = Guarded(ctx, 808)
    d_sel = None
    if select is not None:
        d_sel = ctx.alloc(max(16, select.nbytes))
        d_sel.upload(select)
    try:
        ctx.flow_fanout_device(batch, opts, res.ptr, select=d_sel, stream=stream,
                               **{k: bufs[k].ptr for k in outputs})
        if stream is not None:
            ctx.stream_synchronize(stream)
        ctx.synchronize()
        got = {"result": abi.FanoutResult.from_bytes(res.read()).as_dict()}
        assert got["result"] == want["result"], f"{where}: result " + ", ".join(
            k for k in want["result"] if got["result"][k] != want["result"][k])
        ns = want["result"]["n_selected"]
        for k in outputs:
            raw = bufs[k].read()
            if k == "hash":
                got[k] = raw.view(np.uint32)
            elif k == "queue":
                got[k] = raw
            elif k == "idx":
                got[k] = raw.view(np.uint32)[:ns]
                assert (raw[4 * ns:] == POISON).all(), f"{where}: idx written at or past n_selected"
            else:
                got[k] = raw.view(np.uint64)
            bad = np.nonzero(got[k] != want[k])[0]
            assert len(got[k]) == len(want[k]) and len(bad) == 0, f"{where}: {k} differs at {bad[:8]}"
        return got
    finally:
        for b in list(bufs.values()) + [res] + ([d_sel] if d_sel else []):
            b.free()


def golden_want(name, src, opts_key, queues, reta=None, select=None, l3_only=False):
    h, k = golden_keys(name, KEYS[opts_key][2], l3_only)
    return fr.expected(h[src.reps], k[src.reps], src.lens, queues, reta, select)


@pytest.mark.parametrize("n", SIZES)
def test_sizes_at_tile_and_chunk_edges(gpu_ctx, n):
    for name, kind in (("fuzz", "random"), ("c4", "null")):
        src = Source(gpu_ctx, name, n)
        try:
            sel = select_words(kind, n)
            run(gpu_ctx, src.batch, n, make_opts(8), golden_want(name, src, "default", 8, select=sel), sel,
                where=f"{name} n={n}")
        finally:
            src.free()


@pytest.mark.parametrize("queues", [1, 3, 8, 64])
@pytest.mark.parametrize("name", ["c3", "c4", "edge", "fuzz"])
def test_contents(gpu_ctx, name, queues):
    """Keys default / symmetric / user, reta default / everything on two queues, five selections."""
    g, _ = load_golden(name)
    n = len(g["desc"])
    src = Source(gpu_ctx, name, n)
    two = [(i * 7 + 3) % 2 * (queues - 1) for i in range(128)]   # queues 0 and K - 1
    try:
        for key in KEYS:
            for reta in (None, two):
                for kind in ("null", "ones", "zeros", "random", "verdict"):
                    sel = select_words(kind, n, g["code__c3"] == 0, seed=queues)
                    want = golden_want(name, src, key, queues, reta, sel)
                    run(gpu_ctx, src.batch, n, make_opts(queues, key, reta), want, sel,
                        where=f"{name} K={queues} {key} reta={'two' if reta else 'default'} {kind}")
    finally:
        src.free()


def test_l3_only(gpu_ctx):
    src = Source(gpu_ctx, "fuzz", 8192)
    try:
        run(gpu_ctx, src.batch, 8192, make_opts(8, l3_only=True), golden_want("fuzz", src, "default", 8, l3_only=True))
    finally:
        src.free()


def test_optional_outputs_alone_and_none(gpu_ctx):
    n = 16384 + 77
    src = Source(gpu_ctx, "fuzz", n)
    sel = select_words("random", n)
    want = golden_want("fuzz", src, "default", 8, select=sel)
    try:
        for outs in ((), ("hash",), ("queue",), ("idx",), ("select_q",)):
            run(gpu_ctx, src.batch, n, make_opts(8), want, sel, outputs=outs, where=f"outputs={outs}")
    finally:
        src.free()


def test_fixed_stride_c1(gpu_ctx):
    g, _ = load_golden("c1")
    n = len(g["rec"])
    assert len(g["data"]) == 64 * n
    d = gpu_ctx.alloc(64 * n)
    try:
        d.upload(g["data"])
        h, k = golden_keys("c1", fr.DEFAULT_KEY)
        want = fr.expected(h, k, np.full(n, 64), 8)
        run(gpu_ctx, abi.Batch(d.ptr, None, 64, n, 0, 0, 0), n, make_opts(8), want, where="c1 stride 64")
    finally:
        d.free()


def test_xdp_descriptors(gpu_ctx):
    n = 2048 + 5
    src = Source(gpu_ctx, "c4", n, xdp=True)
    try:
        sel = select_words("random", n)
        run(gpu_ctx, src.batch, n, make_opts(8, "symmetric"), golden_want("c4", src, "symmetric", 8, select=sel), sel)
    finally:
        src.free()


def test_frames_running_past_bytes_read_zeros(gpu_ctx):
    """The last frames' descriptors run past `bytes`: their missing bytes read as zeros. Expected
    values from the Python walk over the zero-extended bytes."""
    g, _ = load_golden("c4")
    n = 300
    desc = g["desc"][:n]
    off, ln = (desc & fr.MASK48).astype(np.int64), (desc >> np.uint64(48)).astype(np.int64)
    assert (np.diff(off) > 0).all()
    for cut in (int(off[290]) + 30, int(off[280]) + 64, int(off[295]) + 16):
        data = g["data"][:int(off[-1] + ln[-1])].copy()
        data[cut:] = 0
        frames = [data[o:o + k] for o, k in zip(off, ln)]
        inputs, nbytes, klass = fr.key_of_frames(frames)
        assert (klass[296:] == fr.NONE).all() and klass[0] != fr.NONE
        want = fr.expected(fr.toeplitz_many(fr.DEFAULT_KEY, inputs, nbytes), klass, ln, 8)
        src = Source(gpu_ctx, "c4", n, data=data[:cut], desc=desc, nbytes=cut)
        try:
            run(gpu_ctx, src.batch, n, make_opts(8), want, where=f"cut={cut}")
        finally:
            src.free()


def test_behind_parse_filter_on_one_stream(gpu_ctx, manifest):
    """select = the verdict words bt_parse_filter_device writes on the same stream, no synchronisation between."""
    g, _ = load_golden("c3")
    n = 16384 + 4096
    src = Source(gpu_ctx, "c3", n)
    gpu_ctx.compile(manifest["filter_sets"]["c3"])
    ntiles = (n + 63) // 64
    d_ver, d_dec = gpu_ctx.alloc(8 * ntiles), gpu_ctx.alloc(n)
    st = gpu_ctx.stream_create()
    bufs = {k: Guarded(gpu_ctx, s) for k, s in (("idx", 4 * n), ("select_q", 8 * 8 * ntiles), ("result", 808))}
    try:
        passed = np.resize(g["code__c3"] == 0, n)
        want = golden_want("c3", src, "default", 8, select=fr.pack_bits(passed))
        gpu_ctx.run_device(src.batch, abi.Outputs(None, 0, d_ver.ptr, d_dec.ptr, None, None), st)
        gpu_ctx.flow_fanout_device(src.batch, make_opts(8), bufs["result"].ptr, select=d_ver, idx=bufs["idx"].ptr,
                                   select_q=bufs["select_q"].ptr, stream=st)
        gpu_ctx.stream_synchronize(st)
        assert abi.FanoutResult.from_bytes(bufs["result"].read()).as_dict() == want["result"]
        assert 0 < want["result"]["n_selected"] < n
        assert (bufs["idx"].read(np.uint32)[:len(want["idx"])] == want["idx"]).all()
        assert (bufs["select_q"].read(np.uint64) == want["select_q"]).all()
    finally:
        gpu_ctx.stream_destroy(st)
        gpu_ctx.compile([])
        for b in list(bufs.values()) + [d_ver, d_dec]:
            b.free()
        src.free()


def _tcp(src, dst, sp, dp):
    ip = bytes([0x45, 0, 0, 40, 0, 0, 0, 0, 64, 6, 0, 0]) + bytes(src) + bytes(dst)
    return bytes(12) + b"\x08\x00" + ip + sp.to_bytes(2, "big") + dp.to_bytes(2, "big") + bytes(16)


def _crafted(ctx, frames, n):
    """n descriptors over the frames (repeated in order), each frame at an odd offset."""
    data, offs = bytearray(), []
    for f in frames:
        data += bytes(-len(data) % 4 + 1)   # the next frame starts at 1 mod 4
        offs.append(len(data))
        data += f
    desc = np.array([o | len(f) << 48 for o, f in zip(offs, frames)], np.uint64)
    return Source(ctx, "c3", n, data=np.frombuffer(bytes(data), np.uint8), desc=desc)


def test_one_flow_fills_one_queue_across_chunks(gpu_ctx):
    n = 2 * 16384 + 5
    f = _tcp([10, 1, 2, 3], [10, 3, 2, 1], 40000, 443)
    src = _crafted(gpu_ctx, [f], n)
    try:
        h = fr.toeplitz(fr.DEFAULT_KEY, fr.walk(f)[0])
        want = fr.expected(np.full(n, h, np.uint32), np.full(n, fr.V4_L4), src.lens, 8)
        assert max(np.diff(want["result"]["start"])) == n
        got = run(gpu_ctx, src.batch, n, make_opts(8), want)
        assert (got["idx"] == np.arange(n)).all()
    finally:
        src.free()


def test_a_wave_with_64_distinct_queues(gpu_ctx):
    """K = 64 with a user reta and tuples chosen so that the 64 packets of every tile hit 64 queues."""
    reta = [(i * 29 + 5) % 64 for i in range(128)]
    frames, used, sp = [], set(), 1024
    while len(frames) < 192:
        f = _tcp([192, 168, 7, 9], [172, 16, 0, 1], sp, 80)
        sp += 1
        q = reta[fr.toeplitz(fr.DEFAULT_KEY, fr.walk(f)[0]) & 127]
        if q not in used:
            used.add(q)
            frames.append(f)
            if len(used) == 64:
                used = set()
    n = 16384 + 192
    src = _crafted(gpu_ctx, frames, n)
    try:
        inputs, nbytes, klass = fr.key_of_frames(frames)
        h = fr.toeplitz_many(fr.DEFAULT_KEY, inputs, nbytes)
        want = fr.expected(h[src.reps], klass[src.reps], src.lens, 64, reta)
        assert len(set(want["queue"][:64].tolist())) == 64 and min(np.diff(want["result"]["start"])) > 0
        run(gpu_ctx, src.batch, n, make_opts(64, reta=reta), want)
    finally:
        src.free()


def test_partition_property(gpu_ctx):
    n = 16384 + 999
    src = Source(gpu_ctx, "fuzz", n)
    try:
        sel = select_words("random", n)
        got = run(gpu_ctx, src.batch, n, make_opts(8), golden_want("fuzz", src, "default", 8, select=sel), sel)
    finally:
        src.free()
    bits = fr.select_bits(sel, n)
    start, idx = got["result"]["start"], got["idx"].astype(np.int64)
    assert sorted(idx.tolist()) == np.nonzero(bits)[0].tolist()
    rows = got["select_q"].reshape(8, -1)
    acc = np.zeros(rows.shape[1], np.uint64)
    for q in range(8):
        part = idx[start[q]:start[q + 1]]
        assert (np.diff(part) > 0).all()
        assert (acc & rows[q]).max(initial=0) == 0
        acc |= rows[q]
        assert np.nonzero(fr.select_bits(rows[q], rows.shape[1] * 64))[0].tolist() == part.tolist()
    assert (acc == fr.pack_bits(bits)).all()


def test_rows_compose_with_the_pack(gpu_ctx):
    """Row q of select_q as bt_pass_pack_device's select (lead 0, align 1) = the numpy pack of queue q's frames."""
    g, _ = load_golden("c4")
    n, queues = 2048, 8
    src = Source(gpu_ctx, "c4", n)
    ntiles = n // 64
    d_rows, d_res = gpu_ctx.alloc(8 * queues * ntiles), gpu_ctx.alloc(808)
    d_out, d_tot, d_np = gpu_ctx.alloc(len(g["data"]) + 64), gpu_ctx.alloc(8), gpu_ctx.alloc(4)
    try:
        gpu_ctx.flow_fanout_device(src.batch, make_opts(queues), d_res, select_q=d_rows)
        gpu_ctx.synchronize()
        res = abi.FanoutResult.from_bytes(d_res.download(np.zeros(808, np.uint8))).as_dict()
        want = golden_want("c4", src, "default", queues)
        assert res == want["result"]
        off = (src.desc & fr.MASK48).astype(np.int64)
        for q in range(queues):
            mine = np.nonzero(want["queue"] == q)[0]
            packed = np.concatenate([g["data"][off[i]:off[i] + src.lens[i]] for i in mine])
            assert len(packed) == res["bytes"][q] > 0
            gpu_ctx.pass_pack(src.batch, d_rows.ptr + 8 * q * ntiles, d_out, len(packed), d_tot, d_np)
            gpu_ctx.synchronize()
            assert int(d_tot.download(np.zeros(1, np.uint64))[0]) == len(packed)
            assert int(d_np.download(np.zeros(1, np.uint32))[0]) == len(mine) == res["start"][q + 1] - res["start"][q]
            assert (d_out.download(np.zeros(d_out.nbytes, np.uint8))[:len(packed)] == packed).all()
    finally:
        for b in (d_rows, d_res, d_out, d_tot, d_np):
            b.free()
        src.free()


def test_two_runs_are_byte_equal(gpu_ctx):
    n = 3 * 16384 + 17
    src = Source(gpu_ctx, "fuzz", n)
    try:
        sel = select_words("random", n)
        want = golden_want("fuzz", src, "default", 64, select=sel)
        a = run(gpu_ctx, src.batch, n, make_opts(64), want, sel)
        b = run(gpu_ctx, src.batch, n, make_opts(64), want, sel)
        assert a["result"] == b["result"] and all((a[k] == b[k]).all() for k in OUTPUTS)
    finally:
        src.free()


def _ab_contents(ctx):
    for name, queues, key in (("fuzz", 8, "default"), ("c4", 64, "user"), ("edge", 3, "symmetric")):
        n = 16384 + 321
        src = Source(ctx, name, n)
        try:
            sel = select_words("random", n)
            run(ctx, src.batch, n, make_opts(queues, key), golden_want(name, src, key, queues, select=sel), sel,
                where=f"A/B {name}")
        finally:
            src.free()


def test_the_other_toeplitz_form_gives_the_same_contents():
    """BT_FANOUT_TABLE=0 (bit-serial, key in SGPRs) in a child process: the knob is read once per process."""
    env = dict(os.environ, BT_FANOUT_TABLE="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "fanout contents hold" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


if __name__ == "__main__":
    c = abi.Context(0)
    try:
        _ab_contents(c)
    finally:
        c.close()
    print(f"fanout contents hold (BT_FANOUT_TABLE={os.environ.get('BT_FANOUT_TABLE', '')})")
