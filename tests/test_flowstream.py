"""CPU: per-flow stream matching on the host (bt_flow_stream_host, bt_flow_stream_compile) against the
restatement in flowstream_ref.py (streams as Python bytes, matches by `re`), the compile's and the
entry points' refusals (decided before the context, so with a null one), `hit` in place of `select`,
and the hits against bt_payload_dfa_search over the concatenated streams' prefixes."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flowstream_cases as fc  # noqa: E402
import flowstream_ref as sr  # noqa: E402
from beatrice_amd import abi  # noqa: E402

BIDIR = 2
BT_E_INVALID_ARGUMENT, BT_E_NOT_IMPLEMENTED = 1, 11


def lay_out(frames):
    """(data, packed descriptors): every frame at an odd offset, 64 zero bytes behind the last."""
    data, desc = bytearray(), []
    for f in frames:
        data += bytes(-len(data) % 4 + 1)
        desc.append(len(data) | len(f) << 48)
        data += f
    data += bytes(64)
    return np.frombuffer(bytes(data), np.uint8), np.array(desc, np.uint64)


def words_of(bits):
    w = np.zeros((len(bits) + 63) // 64, np.uint64)
    for i, b in enumerate(bits):
        if b:
            w[i >> 6] |= np.uint64(1 << (i & 63))
    return w


def host_against_ref(pattern, blob, batches, cap, flags, start=None):
    """Every batch through the host form and through the restatement, from the same table; returns the
    restatement (its table and streams) and the hit words per batch."""
    model = sr.Streams(cap, pattern, blob, flags, start)
    table = (np.zeros(cap, abi.FlowStreamRec) if start is None else start.copy().view(abi.FlowStreamRec))
    hits = []
    for k, (frames, ids, bits) in enumerate(batches):
        data, desc = lay_out(frames)
        sel = None if all(bits) else words_of(bits)
        if sel is not None and len(frames) % 64:
            sel[-1] |= ~np.uint64(0) << np.uint64(len(frames) % 64)   # must be ignored
        want_hit, want_res = model.batch(frames, ids, sel)
        hit = np.full((len(frames) + 63) // 64, 0xDEADBEEF, np.uint64)
        res = abi.flow_stream_host(data, desc, np.array(ids, np.uint32), sel, flags, blob, table, hit=hit)
        res.pop("reserved", None)
        assert res == want_res, f"batch {k}: result {res} != {want_res}"
        bad = [i for i in range(len(frames)) if (int(hit[i >> 6]) ^ int(want_hit[i >> 6])) >> (i & 63) & 1]
        assert not bad and (hit == want_hit).all(), f"batch {k}: hit differs at packets {bad[:8]}"
        assert table.tobytes() == model.table.tobytes(), f"batch {k}: table"
        hits.append(hit)
    return model, hits


@pytest.mark.parametrize("flags", [0, BIDIR])
@pytest.mark.parametrize("case", fc.PATTERNS, ids=[p[0] for p in fc.PATTERNS])
def test_host_form_against_the_restatement(case, flags):
    pattern, positions, text = case
    blob, info = abi.flow_stream_compile(pattern)
    assert info["positions"] == positions and info["tail"] == positions - 1 and info["width"] >= positions
    rows, cap = fc.crafted(text, info["tail"])
    model, _ = host_against_ref(pattern, blob, fc.batches_of(rows), cap, flags)
    assert int(model.table["hit_packets"].sum()) > len(text)   # the cut points alone give len - 1 hits


def test_the_named_cases_say_what_they_mean():
    """GE + T / in two segments hits the second; a match wholly in the tail does not hit again; halves in
    the two directions meet only when the table has no directions."""
    blob, info = abi.flow_stream_compile("GET /")
    for flags, across in ((0, True), (BIDIR, False)):
        frames = [fc.frame(b"GE"), fc.frame(b"T / HTTP"), fc.frame(b"x"), fc.frame(b"GET"), fc.reply(b" /")]
        _, hits = host_against_ref("GET /", blob, [(frames, [0, 0, 0, 1, 1], [True] * 5)], 2, flags)
        assert int(hits[0][0]) == (0b10010 if across else 0b00010)


def test_a_starting_table_with_a_state():
    """A table whose d holds any bits of the pattern's positions: the state and the hits follow from the
    Shift-And step alone."""
    pattern, positions, text = fc.PATTERNS[3]
    blob, info = abi.flow_stream_compile(pattern)
    rng = np.random.default_rng(5)
    start = np.zeros(8, sr.STREAM_REC)
    start["d"] = rng.integers(0, 1 << positions, (8, 2), dtype=np.uint64)
    start["hit_packets"][::2, 0] = 3
    start["stream_packets"][:] = 0xFFFFFFFF   # wraps
    frames = [fc.frame(text[k:]) for k in range(8)] + [fc.reply(text[k:]) for k in range(8)]
    model, _ = host_against_ref(pattern, blob, [(frames, list(range(8)) * 2, [True] * 16)], 8, BIDIR, start)
    assert int(model.table["stream_packets"][0][0]) == 0


def test_random_streams_and_hits_against_the_searched_prefixes():
    pattern, _, text = fc.PATTERNS[0]
    blob, info = abi.flow_stream_compile(pattern)
    rng = np.random.default_rng(11)
    cap, batches = 5, []
    for b in range(3):
        frames, ids = [], []
        for i in range(300):
            ln = int(rng.choice([0, 1, 2, 3, 5, 9, 40]))
            mk = fc.frame if rng.integers(0, 2) else fc.reply
            frames.append(mk(fc.filler(ln, text, 1000 * b + i), proto=int(rng.choice([6, 17]))))
            ids.append(int(rng.choice([0, 1, 2, 3, 4, 5, 0xFFFFFFFE])))
        batches.append((frames, ids, [bool(x) for x in rng.integers(0, 4, 300)]))
    model, hits = host_against_ref(pattern, blob, batches, cap, BIDIR)
    assert model.table["hit_packets"].sum() > 20
    # over the concatenated stream: some packet up to a boundary is hit iff the search finds a match in the prefix
    seen, any_hit = {}, {}
    for (frames, ids, bits), hit in zip(batches, hits):
        for i, (f, fid, on) in enumerate(zip(frames, ids, bits)):
            pl = sr.payload_of(f)
            if not on or fid >= cap or pl is None:
                continue
            key = (fid, sr.direction(f, BIDIR))
            seen[key] = seen.get(key, b"") + f[pl[0]:pl[1]]
            any_hit[key] = any_hit.get(key, False) or bool(int(hit[i >> 6]) >> (i & 63) & 1)
            assert any_hit[key] == abi.payload_dfa_search(bytes(blob), seen[key]), (key, i)


def test_hit_may_be_select():
    blob, _ = abi.flow_stream_compile("GET|POST")
    frames = [fc.frame(b"GE"), fc.frame(b"T"), fc.frame(b"POST"), fc.frame(b"POST")] * 40
    data, desc = lay_out(frames)
    ids = np.arange(len(frames), dtype=np.uint32) // 2
    sel = words_of([i % 4 != 2 for i in range(len(frames))])
    apart, t1 = np.zeros_like(sel), np.zeros(80, abi.FlowStreamRec)
    r1 = abi.flow_stream_host(data, desc, ids, sel.copy(), 0, blob, t1, hit=apart)
    both, t2 = sel.copy(), np.zeros(80, abi.FlowStreamRec)
    r2 = abi.flow_stream_host(data, desc, ids, both, 0, blob, t2, hit=both)
    assert r1 == r2 and (apart == both).all() and t1.tobytes() == t2.tobytes() and r1["hit_packets"] == 80
    assert abi.decode_flow_stream(t1[0]) == {"state": [int(t1[0]["d"][0]), 0], "stream_packets": [2, 0], "hit_packets": [1, 0], "hit": True}


@pytest.mark.parametrize("pattern,word", fc.REFUSED)
def test_the_compile_refuses_by_construct(pattern, word):
    with pytest.raises(abi.BtError) as e:
        abi.flow_stream_compile(pattern)
    assert e.value.args and f"error {BT_E_NOT_IMPLEMENTED}:" in str(e.value) and word in str(e.value), str(e.value)


@pytest.mark.parametrize("pattern", fc.NOT_A_REGEX)
def test_the_compile_rejects_what_std_regex_rejects(pattern):
    with pytest.raises(abi.BtError) as e:
        abi.flow_stream_compile(pattern)
    assert f"error {BT_E_INVALID_ARGUMENT}:" in str(e.value)


def test_refusals_need_no_gpu():
    """Every refusal is decided before the context is looked at: with a null context each one is reported
    by its own reason, the null context last."""
    L = abi.lib()
    blob, _ = abi.flow_stream_compile("GET|POST")
    other = np.frombuffer(abi.payload_dfa("GET.+"), np.uint8).copy()   # a blob the PAYLOAD filter takes and this matcher does not
    data = (ctypes.c_uint8 * 256)()
    desc = (ctypes.c_uint64 * 4)()
    ids = (ctypes.c_uint32 * 4)()
    table = (ctypes.c_uint64 * 16)()
    res = (ctypes.c_uint64 * 8)()
    words = (ctypes.c_uint64 * 2)()
    raw = (ctypes.c_uint8 * (1 << 17))()
    ip, tp, rp, wp = (ctypes.addressof(x) for x in (ids, table, res, words))
    sp = (ctypes.addressof(raw) + 255) & ~255
    need = abi.flow_stream_scratch_bytes(2, 4)
    assert 0 < need <= (1 << 17) - 256 and abi.flow_stream_scratch_bytes(0, 0) >= 256
    bp = blob.ctypes.data

    def said(rc, word, code=BT_E_INVALID_ARGUMENT):
        msg = L.bt_last_error().decode()
        assert rc == code and word in msg, (word, rc, msg)

    def good():
        return abi.Batch(ctypes.addressof(data), ctypes.addressof(desc), 0, 2, 256, abi.DESC_PACKED, 0)

    def out_of(hit=wp, result=rp, reserved=(0, 0)):
        return abi.FlowStreamOut(hit, result, (ctypes.c_uint64 * 2)(*reserved))

    def dev(word, frames, flow_id=ip, select=wp, flags=0, pat=bp, pat_dev=bp, pat_bytes=len(blob), tab=tp, cap=4, scratch=sp,
            nbytes=need, out=out_of(), code=BT_E_INVALID_ARGUMENT):
        said(L.bt_flow_stream_device(None, ctypes.byref(frames) if frames is not None else None, flow_id, select, flags, pat, pat_dev,
                                     pat_bytes, tab, cap, scratch, nbytes, ctypes.byref(out) if out is not None else None, None), word, code)

    dev("bt_flow_stream_device: null context", good())
    dev("null context", good(), select=None, out=out_of(hit=None), flags=3)
    dev("null frames", None)
    dev("null out", good(), out=None)
    dev("null result", good(), out=out_of(result=None))
    dev("unknown flag", good(), flags=4)
    for k in range(2):
        dev("reserved is not 0", good(), out=out_of(reserved=[int(j == k) for j in range(2)]))
    dev("null flow_id", good(), flow_id=None)
    dev("null table", good(), tab=None)
    dev("flow_id is not 4-byte aligned", good(), flow_id=ip + 2)
    dev("table is not 8-byte aligned", good(), tab=tp + 4)
    dev("select is not 8-byte aligned", good(), select=wp + 4)
    dev("hit is not 8-byte aligned", good(), out=out_of(hit=wp + 4))
    dev("result is not 8-byte aligned", good(), out=out_of(result=rp + 4))
    dev("flow_cap above 2^31", good(), cap=(1 << 31) + 1)
    dev("null pattern_device", good(), pat_dev=None)
    dev("pattern_device is not 8-byte aligned", good(), pat_dev=bp + 4)
    dev("scratch is not 256-byte aligned", good(), scratch=sp + 8)
    for flag in (abi.BATCH_PREFIXES, abi.BATCH_LEAN):
        f = good()
        f.flags = flag
        dev("BT_BATCH_PREFIXES", f)
    f = good()
    f.bytes = 0
    dev("bytes == 0", f)
    dev("null pattern", good(), pat=None)
    dev("below a blob's header", good(), pat_bytes=40)
    dev("below the blob's table", good(), pat_bytes=len(blob) - 1)
    dev("repeatable", good(), pat=other.ctypes.data, pat_bytes=len(other), code=BT_E_NOT_IMPLEMENTED)
    dev("null scratch", good(), scratch=None)
    dev("scratch_bytes", good(), nbytes=need - 1)
    f = good()
    f.n = 0
    dev("null context", f, flow_id=None, tab=None, cap=0, scratch=None, nbytes=0)   # an empty batch needs none of them

    def host(word, base=ctypes.addressof(data), d=ctypes.addressof(desc), flow_id=ip, select=wp, flags=0, pat=bp, pat_bytes=len(blob),
             tab=tp, cap=4, out=out_of(), code=BT_E_INVALID_ARGUMENT):
        said(L.bt_flow_stream_host(base, 256, d, 2, flow_id, select, flags, pat, pat_bytes, tab, cap,
                                   ctypes.byref(out) if out is not None else None), word, code)

    host("bt_flow_stream_host: null base / desc", d=None)
    host("null out", out=None)
    host("null result", out=out_of(result=None))
    host("unknown flag", flags=0x80000000)
    host("reserved is not 0", out=out_of(reserved=(0, 7)))
    host("null flow_id", flow_id=None)
    host("null table", tab=None)
    host("hit is not 8-byte aligned", out=out_of(hit=wp + 4))
    host("null pattern", pat=None)
    host("repeatable", pat=other.ctypes.data, pat_bytes=len(other), code=BT_E_NOT_IMPLEMENTED)
    # nothing was written by any refused call
    assert not any(table) and not any(res) and not any(words)


def test_an_empty_batch_writes_the_result():
    blob, _ = abi.flow_stream_compile("GET|POST")
    table = np.zeros(3, abi.FlowStreamRec)
    res = abi.flow_stream_host(np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32), None, 0, blob, table)
    assert res["n"] == 0 and res["selected"] == 0 and res["stream_bytes"] == 0 and not table.view(np.uint64).any()


def test_flowstream_host_check_builds_and_passes(tmp_path):
    """tools/flowstream_host_check.cpp: the predicate, the argument checks and the host form against a naive
    oracle (each stream concatenated in a std::map, std::regex on every window that ends inside a packet)
    under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program."""
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "flowstream_host_check")
    # the sanitizer runtimes linked into the program: it runs the same whatever else a process preloads
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-I" + os.path.join(root, "include"), "-I" + os.path.join(root, "beatrice_amd", "csrc"),
                    os.path.join(root, "tools", "flowstream_host_check.cpp"), os.path.join(root, "beatrice_amd", "csrc", "bt_regex_dfa.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all cases hold" in r.stdout, r.stdout + r.stderr
