"""GPU: the second pass of the PAYLOAD filter (bt_filter_resume_device, bt_payload_resume.hip).
A batch first run with BATCH_PREFIXES leaves DECIDE_HOST at every GPU PAYLOAD slot a frame
reaches; the resume pass over the whole frames of the same batch finishes those chains on the
device, after which the decision bytes, verdict words and pass list equal the single whole-frame
pass and the compiled reference (goldens; oracle/_ref where built)."""
import json
import os

import numpy as np
import pytest

import oracle_lib as ol
from beatrice_amd import abi, synth
from conftest import GOLDEN, load_golden
from golden_util import compare_decisions

pytestmark = pytest.mark.gpu

# tests/test_gpu_payload.py's list: every blob form (bit-parallel 32 / 64-bit, anchors, byte DFA)
FORM_PATTERNS = ["GET|POST", "User-Agent: .*(bot|curl)", "^.{0,5}$", "\\s+$", "[\\x80-\\xff]{4,}", "passw(or)?d=",
                 "^\\x16\\x03[\\x00-\\x03]", "(?:GET|HEAD) /[^ ]* HTTP", "a.?b*c", "[0-9a-f]{2}[^a-z]?z+$"]
THROWING_IP = "10.0.0.0/99999999999"


def _single(ctx, data, desc, n):
    run = abi.DeviceRun(ctx, data, desc, n, records=False)
    run.run()
    out = run.fetch()
    run.free()
    return out


def _two_pass(ctx, data, desc, n, verdict=True):
    """(first-pass decision bytes, outputs after the resume pass) of one descriptor batch: the
    first pass with BATCH_PREFIXES over the whole-frame data (the flag alone keeps the payload
    unread), the resume pass over the same batch with flags 0. A caller's verdict words are
    overwritten in between, so every word read afterwards was rebuilt by the resume pass."""
    run = abi.DeviceRun(ctx, data, desc, n, records=False, verdict=verdict)
    try:
        run.batch.flags = abi.BATCH_PREFIXES
        run.run()
        first = run.fetch()["decide"].copy()
        run.batch.flags = 0
        if run.d_ver:
            run.d_ver.upload(np.full(run.d_ver.nbytes, 0xA5, np.uint8))
        ctx.resume_device(run.batch, run.outs)
        out = run.fetch()
    finally:
        run.free()
    return first, out


def _kinds(prog):
    return [abi.KINDS[s.kind] for s in prog]


def _host_at(decide, slot):
    return ((decide >> 6) == abi.DECIDE_HOST) & ((decide & 63) == slot)


def _check_outputs(out, n):
    """Verdict words and the pass list against the decision bytes."""
    want = (out["decide"] >> 6) == abi.DECIDE_PASS
    if "verdict" in out:
        bits = np.unpackbits(out["verdict"].view(np.uint8), bitorder="little")
        assert np.array_equal(bits[:n].astype(bool), want) and not bits[n:].any()
    assert out["n_pass"] == int(want.sum())
    assert np.array_equal(out["pass_idx"], np.nonzero(want)[0])


def test_goldens_default_context(gpu_ctx):
    g, man = load_golden("http")
    n = len(g["desc"])
    both = 0
    sets = [s for s in dict.fromkeys(man["captures"]["http"]["filter_sets"]) if s.startswith("payload_")]
    assert "payload_chain" in sets and "payload_host_mix" in sets
    for s in sets:
        filters = man["filter_sets"][s]
        prog = gpu_ctx.compile(filters)
        first, out = _two_pass(gpu_ctx, g["data"], g["desc"], n)
        dec = out["decide"]
        compare_decisions(dec, g[f"code__{s}"], g[f"src__{s}"], filters, where=f"http/{s} resumed")
        kinds = _kinds(prog)
        for k, kind in enumerate(kinds):
            if kind == "PAYLOAD":
                assert not _host_at(dec, k).any(), f"{s}: HOST left at GPU slot {k}"
        if "PAYLOAD" in kinds:
            assert _host_at(first, kinds.index("PAYLOAD")).any(), f"{s}: the first pass left no work"
        host_slots = set((dec & 63)[(dec >> 6) == abi.DECIDE_HOST].tolist())
        assert all(kinds[k] == "HOST" for k in host_slots), f"{s}: HOST codes at {host_slots}"
        if s == "payload_host_mix":
            assert host_slots, "payload_host_mix: the host slots decide nothing"
        code = g[f"code__{s}"]
        both += int((code == 0).any() and (code == 1).any())
        _check_outputs(out, n)
    assert both >= 17
    assert np.bincount(g["code__payload_re_0"], minlength=2)[:2].tolist() == [528, 2472]
    assert np.bincount(g["code__payload_chain"], minlength=2)[:2].tolist() == [192, 2808]


def test_goldens_extended_context():
    z = np.load(os.path.join(GOLDEN, "regex_ext.npz"), allow_pickle=False)
    g = {k: z[k] for k in z.files}
    with open(os.path.join(GOLDEN, "regex_ext.json")) as fh:
        meta = json.load(fh)
    n = len(g["desc"])
    assert n == 1588 and len(meta["patterns"]) == 37
    ctx = abi.Context(0, flags=abi.OPT_PAYLOAD_EXTENDED)
    try:
        for p, expr in enumerate(meta["patterns"]):
            f = [{"type": abi.PAYLOAD, "expr": expr, "priority": 1}]
            assert _kinds(ctx.compile(f)) == ["PAYLOAD"], f"/{expr}/ stayed on the host"
            first, out = _two_pass(ctx, g["data"], g["desc"], n)
            assert _host_at(first, 0).all(), f"/{expr}/: first pass"
            assert not ((out["decide"] >> 6) == abi.DECIDE_HOST).any(), f"/{expr}/: HOST codes left"
            compare_decisions(out["decide"], g["code"][p], g["src"][p], f, where=f"regex_ext /{expr}/ resumed")
            assert min(int((g["code"][p] == 0).sum()), int((g["code"][p] == 1).sum())) >= 54
        assert _kinds(ctx.compile(meta["chain"])) == ["PROTO_EQ", "PAYLOAD", "PAYLOAD", "PORT"]
        first, out = _two_pass(ctx, g["data"], g["desc"], n)
        assert _host_at(first, 1).any() and not ((out["decide"] >> 6) == abi.DECIDE_HOST).any()
        compare_decisions(out["decide"], g["chain_code"], g["chain_src"], meta["chain"], where="regex_ext chain resumed")
        _check_outputs(out, n)
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def fuzz_forms():
    """A 4,096-frame FUZZ capture with pattern-shaped text planted in every 5th frame's payload,
    and per FORM_PATTERNS expression the host executor's answer per frame."""
    n = 4096
    data, desc = synth.capture(synth.FUZZ, n, seed=77)
    off, ln = synth.desc_off(desc), synth.desc_len(desc)
    words = [b"GET /", b"POST", b"User-Agent: x bot", b"passwd=", b"\x16\x03\x01", b"HEAD /a HTTP", b"abbbc", b"0fzz"]
    for i in range(0, n, 5):
        o, m = int(off[i]), int(ln[i])
        w = words[(i // 5) % len(words)]
        at = o + 14 + 4 * (int(data[o + 14]) & 15 if m > 14 else 5) + (i % 3)
        if at + len(w) <= o + m:
            data[at:at + len(w)] = np.frombuffer(w, np.uint8)
    frames = [data[o:o + m].tobytes() for o, m in zip(off, ln)]
    want = {}
    for expr in FORM_PATTERNS:
        blob = abi.payload_dfa(expr)
        want[expr] = np.array([abi.payload_dfa_eval(blob, f) for f in frames])
    return data, desc, want


@pytest.mark.parametrize("flags", [0, abi.OPT_PAYLOAD_DFA], ids=["bitpar", "dfa"])
def test_every_blob_form(fuzz_forms, flags):
    data, desc, want = fuzz_forms
    n = len(desc)
    ctx = abi.Context(0, flags=flags)
    try:
        for expr in FORM_PATTERNS:
            assert _kinds(ctx.compile([{"type": abi.PAYLOAD, "expr": expr, "priority": 1}])) == ["PAYLOAD"]
            first, out = _two_pass(ctx, data, desc, n)
            assert _host_at(first, 0).all()
            exp = np.where(want[expr], abi.DECIDE_PASS << 6, abi.DECIDE_REJECT << 6).astype(np.uint8)
            bad = np.nonzero(out["decide"] != exp)[0]
            assert len(bad) == 0, f"/{expr}/: {len(bad)} differ from the host executor, first {bad[:5]}"
    finally:
        ctx.close()
    assert sum(0 < int(w.sum()) < n for w in want.values()) >= 8


def _crafted_frames():
    """Frames around every edge of applyPayloadFilter's window [po, po + min(len - po, 100)),
    po = 14 + 4 * IHL: each IHL nibble, lengths on both sides of the window's start and end and of
    the 34-byte gate, non-IPv4 EtherTypes, and MAGIC at window offsets 0, 95, 99 (cut by the
    window's end) and 100 (outside)."""
    rng = np.random.default_rng(20)
    frames = []
    for ihl in range(16):
        po = 14 + 4 * ihl
        for ln in (po - 1, po, po + 1, po + 99, po + 100, po + 101, 33, 34, po + 140, po + 180):
            for at in (0, 95, 99, 100, None):
                for v in range(4):
                    f = bytearray(rng.integers(0, 256, ln, dtype=np.uint8).tobytes())
                    i = len(frames)
                    et = b"\x86\xdd" if i % 11 == 5 else b"\x81\x00" if i % 11 == 9 else b"\x08\x00"
                    f[12:14] = et
                    if ln > 14:
                        f[14] = 0x40 | ihl
                    if ln > 23:
                        f[23] = 6 if v & 1 else 17
                    if ln >= 38:
                        f[34:38] = int(rng.integers(0, 65536)).to_bytes(2, "big") + \
                                   int(rng.integers(0, 65536)).to_bytes(2, "big")
                    if v & 2 and po + 3 <= ln:      # `^..?\d`: a digit at window offset 1
                        f[po + 1] = 0x30 + i % 10
                    elif po + 3 <= ln:
                        f[po + 1:po + 3] = b"xy"
                    if at is not None and po + at + 5 <= ln:
                        f[po + at:po + at + 5] = b"MAGIC"
                    frames.append(bytes(f[:ln]))
    return frames


CRAFTED = [{"type": abi.PROTOCOL, "expr": "ip", "priority": 4},
           {"type": abi.PAYLOAD, "expr": "MAG+IC", "priority": 3},
           {"type": abi.PORT_RANGE, "expr": "0-40000", "priority": 2},
           {"type": abi.PAYLOAD, "expr": "^..?\\d", "priority": 1}]


def test_crafted_windows(gpu_ctx):
    frames = _crafted_frames()
    data, desc = synth.pack_frames(frames, align=1)
    n = len(desc)
    off, ln = synth.desc_off(desc), synth.desc_len(desc)
    assert set((off & 15).tolist()) == set(range(16))
    data = data[: int(off[-1] + ln[-1])].copy()      # the last frame ends at the buffer's last byte
    assert set(int(data[o + 14]) & 15 for o, m in zip(off, ln) if m > 14) == set(range(16))
    assert _kinds(gpu_ctx.compile(CRAFTED)) == ["PROTO_NZ", "PAYLOAD", "PORT", "PAYLOAD"]
    first, out = _two_pass(gpu_ctx, data, desc, n)
    dec = out["decide"]
    assert _host_at(first, 1).any() and not ((dec >> 6) == abi.DECIDE_HOST).any()
    single = _single(gpu_ctx, data, desc, n)["decide"]
    bad = np.nonzero(dec != single)[0]
    assert len(bad) == 0, f"{len(bad)} differ from the single pass, first {bad[:5]}: {dec[bad[:5]]} {single[bad[:5]]}"
    if ol.ref_available():
        code, src = ol.ref_filter(data, desc, n, CRAFTED)
        compare_decisions(dec, code, src, CRAFTED, where="crafted windows resumed")
    codes = np.bincount(dec >> 6, minlength=4)
    assert codes[abi.DECIDE_PASS] >= 50 and codes[abi.DECIDE_REJECT] >= 50, codes
    # every slot decides some frame, the last PAYLOAD slot (a window staged once, walked twice) too
    assert set((dec & 63)[(dec >> 6) == abi.DECIDE_REJECT].tolist()) == {0, 1, 2, 3}
    _check_outputs(out, n)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4133])
def test_batch_sizes(gpu_ctx, n):
    g, man = load_golden("http")
    desc = np.resize(g["desc"], n)
    gpu_ctx.compile(man["filter_sets"]["payload_chain"])
    first, out = _two_pass(gpu_ctx, g["data"], desc, n)
    single = _single(gpu_ctx, g["data"], desc, n)
    assert np.array_equal(out["decide"], single["decide"])
    assert np.array_equal(out["verdict"], single["verdict"])
    _check_outputs(out, n)


def test_batch_without_and_with_only_work_items(gpu_ctx):
    g, man = load_golden("http")
    n = len(g["desc"])
    # no PAYLOAD slot: nothing is a work item, decide stays as it is, the outputs are rebuilt
    assert "PAYLOAD" not in _kinds(gpu_ctx.compile(man["filter_sets"]["c3"]))
    first, out = _two_pass(gpu_ctx, g["data"], g["desc"], n)
    assert np.array_equal(first, out["decide"])
    assert np.array_equal(out["decide"], _single(gpu_ctx, g["data"], g["desc"], n)["decide"])
    _check_outputs(out, n)
    # PAYLOAD first: every frame is one, the non-IPv4 and short ones included
    f = [{"type": abi.PAYLOAD, "expr": "GET|POST", "priority": 1}]
    assert _kinds(gpu_ctx.compile(f)) == ["PAYLOAD"]
    first, out = _two_pass(gpu_ctx, g["data"], g["desc"], n)
    assert _host_at(first, 0).all()
    compare_decisions(out["decide"], g["code__payload_re_0"], g["src__payload_re_0"], f, where="all work items")
    assert not ((out["decide"] >> 6) == abi.DECIDE_HOST).any()
    _check_outputs(out, n)


@pytest.mark.parametrize("caller_verdict", [True, False])
def test_verdict_and_pass_list(gpu_ctx, caller_verdict):
    g, man = load_golden("http")
    n = len(g["desc"])
    gpu_ctx.compile(man["filter_sets"]["payload_chain"])
    first, out = _two_pass(gpu_ctx, g["data"], g["desc"], n, verdict=caller_verdict)
    assert ("verdict" in out) == caller_verdict
    _check_outputs(out, n)
    assert out["n_pass"] == 192 and np.all(np.diff(out["pass_idx"].astype(np.int64)) > 0)


def test_throwing_slot_after_payload(gpu_ctx):
    g, man = load_golden("http")
    n = len(g["desc"])
    f = [{"type": abi.PAYLOAD, "expr": "GET|POST", "priority": 3},
         {"type": abi.IP_RANGE, "expr": THROWING_IP, "priority": 2}]
    assert _kinds(gpu_ctx.compile(f)) == ["PAYLOAD", "IP_THROW"]
    first, out = _two_pass(gpu_ctx, g["data"], g["desc"], n)
    dec = out["decide"]
    assert np.array_equal(dec, _single(gpu_ctx, g["data"], g["desc"], n)["decide"])
    thrown = (dec >> 6) == abi.DECIDE_THROW
    assert thrown.sum() == 528 and np.all((dec & 63)[thrown] == 1)    # payload_re_0's passing frames
    assert not ((dec >> 6) == abi.DECIDE_PASS).any()
    _check_outputs(out, n)


def test_refusals(gpu_ctx):
    g, man = load_golden("http")
    n = len(g["desc"])
    gpu_ctx.compile(man["filter_sets"]["payload_chain"])
    run = abi.DeviceRun(gpu_ctx, g["data"], g["desc"], n, records=True)
    try:
        o = run.outs
        ok = abi.Outputs(None, n, o.verdict, o.decide, o.pass_idx, o.n_pass)
        run.batch.flags = abi.BATCH_PREFIXES
        with pytest.raises(abi.BtError, match="BT_BATCH_PREFIXES"):
            gpu_ctx.resume_device(run.batch, ok)
        run.batch.flags = 0
        with pytest.raises(abi.BtError, match="records"):
            gpu_ctx.resume_device(run.batch, o)
        with pytest.raises(abi.BtError, match="decide"):
            gpu_ctx.resume_device(run.batch, abi.Outputs(None, n, o.verdict, None, o.pass_idx, o.n_pass))
        run.batch.bytes = 0
        with pytest.raises(abi.BtError, match="bytes == 0"):
            gpu_ctx.resume_device(run.batch, ok)
    finally:
        run.free()
