"""CPU: the reassembled TCP stream bytes exported on the host (bt_flow_follow_host) behind
bt_flow_tcpseq_host, which gives the offsets: against the restatement in flowfollow_ref.py (bytes, runs,
place, both results, the table); with a pattern against bt_flow_reasm_host byte for byte; for clean
captures against the generator's true streams; for disturbed ones every run against its piece of the true
stream; the capacities; the plain follow without a pattern; the refusals with a null context."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flowfollow_ref as fr  # noqa: E402
import flowreasm_cases as rc  # noqa: E402
import flowreasm_ref as rr  # noqa: E402
from beatrice_amd import abi  # noqa: E402
from test_flowreasm import result_of, select_of  # noqa: E402
from test_flowstream import lay_out, words_of  # noqa: E402

BIDIR = 2
BT_E_INVALID_ARGUMENT = 1
POISON = 0xC7


def follow_result_of(res):
    assert res["reserved"] == 0
    return {k: res[k] for k in fr.FRESULT}


def host_once(data, desc, ids, sel, off, flags, blob, tab, n, cap, run_cap, hit=None, rest=None):
    """bt_flow_follow_host into poisoned outputs of exactly cap bytes and run_cap runs (None: a null pointer).
    Returns (bytes, runs, place, result, follow result)."""
    out = None if cap is None else np.full(cap, POISON, np.uint8)
    runs = None if run_cap is None else np.frombuffer(bytes([POISON]) * (32 * run_cap), abi.FlowFollowRun).copy()
    place = np.full(n, 0x5555, np.uint64)
    res, fres = abi.flow_follow_host(data, desc, ids, sel, off, flags, blob, tab, out_bytes=out, runs=runs, place=place, hit=hit, rest=rest)
    return out, runs, place, res, fres


def check_outputs(at, got, want, cap, run_cap):
    """got: host_once's (or a device call's) outputs; want: the restatement's full bytes, runs, place, fres."""
    out, runs, place, fres = got
    wbytes, wruns, wplace, wfres = want
    assert follow_result_of(fres) == wfres, f"{at}: follow result {fres} != {wfres}"
    w = wfres["written"]
    if cap:
        assert out[:w].tobytes() == wbytes[:w], f"{at}: bytes"
        assert (out[w:] == POISON).all(), f"{at}: bytes written at or past `written`"
    k = wfres["runs_written"]
    if run_cap:
        assert runs[:k].tobytes() == wruns[:k].tobytes(), f"{at}: runs {runs[:k]} != {wruns[:k]}"
        assert runs[k:].tobytes() == bytes([POISON]) * (32 * (run_cap - k)), f"{at}: runs written past runs_written"
    assert (place == wplace).all(), f"{at}: place"


def chain_follow(calls, cap, blob, flags=BIDIR, alias=None, caps=None):
    """Every call through bt_flow_tcpseq_host, then bt_flow_follow_host and the restatement from the same offsets;
    with a pattern, bt_flow_reasm_host from the same table as well. caps: None (enough of both) or a function
    (total, n_runs) -> (cap, run_cap). Returns (the restatement, [(bytes, runs, result, follow result)])."""
    model = fr.Follow(cap, blob, flags)
    seq_tab, tab = np.zeros(cap, abi.FlowTcpseqRec), np.zeros(cap, abi.FlowReasmRec)
    got = []
    for k, rows in enumerate(calls):
        at = f"call {k}"
        n, nw = len(rows), (len(rows) + 63) // 64
        frames, ids = [r.frame for r in rows], np.array([r.flow for r in rows], np.uint32)
        data, desc = lay_out(frames)
        sel = select_of(rows)
        if alias and sel is None:
            sel = words_of([True] * n)
        off = np.full(n, 7, np.int64)
        abi.flow_tcpseq_host(data, desc, ids, sel, flags, seq_tab, off=off)
        before = tab.copy()
        want_hit, want_rest, want_res, wbytes, wruns, wplace, wfres = model.follow(frames, ids, off, sel)
        ocap, rcap = (len(data), n) if caps is None else caps(wfres["total"], wfres["n_runs"])
        wfres = dict(wfres, written=min(wfres["total"], ocap or 0), runs_written=min(wfres["n_runs"], rcap or 0))
        hit, rest = np.full(nw, 0xDEADBEEF, np.uint64), np.full(nw, 0xDEADBEEF, np.uint64)
        use = sel
        if alias == "hit":
            hit = sel.copy()
            use = hit
        elif alias == "rest":
            rest = sel.copy()
            use = rest
        out, runs, place, res, fres = host_once(data, desc, ids, use, off, flags, blob, tab, n, ocap, rcap, hit, rest)
        assert res["reserved0"] == 0 and res["reserved1"] == 0
        assert result_of(res) == want_res, f"{at}: result {result_of(res)} != {want_res}"
        assert (hit == want_hit).all() and (rest == want_rest).all(), f"{at}: hit / rest"
        assert tab.tobytes() == model.table.tobytes(), f"{at}: table"
        check_outputs(at, (out, runs, place, fres), (wbytes, wruns, wplace, wfres), ocap, rcap)
        assert wfres["total"] == want_res["stream_bytes"] == int(wruns["len"].sum())
        if blob is not None:   # the reassembly call from the same inputs: byte-equal
            rtab = before.copy()
            rhit, rrest = np.full(nw, 0xDEADBEEF, np.uint64), np.full(nw, 0xDEADBEEF, np.uint64)
            rres = abi.flow_reasm_host(data, desc, ids, sel, off, flags, blob, rtab, hit=rhit, rest=rrest)
            assert rres == res and rtab.tobytes() == tab.tobytes() and (rhit == hit).all() and (rrest == rest).all(), f"{at}: bt_flow_reasm_host"
        got.append((wbytes, wruns, want_res, wfres))
    return model, got


@pytest.mark.parametrize("flags", [BIDIR, 0])
def test_the_named_cases(flags):
    blob, _ = abi.flow_stream_compile(rc.PATTERN)
    calls, cap, _ = rc.crafted()
    _, got = chain_follow(calls, cap, blob, flags)
    if not flags:
        return
    wbytes, wruns, _, _ = got[0]
    pieces = {int(u["flow"]): [] for u in wruns}
    for u in wruns:
        if not u["flags"] & 1:
            pieces[int(u["flow"])].append((int(u["flags"]), wbytes[int(u["at"]):int(u["at"] + u["len"])]))
    assert pieces[0] == [(fr.NEW, b"abcHELLOdef")]                             # swapped segments, in order
    assert pieces[1] == [(fr.NEW, b"xHELLO")]                                  # three 1-byte segments in reverse
    assert pieces[3] == [(fr.NEW, b"xxHELLOyy")] and pieces[4] == [(fr.NEW, b"xxHELXXyy")]   # the first in (rel, index) order wins
    assert pieces[5] == [(fr.NEW, b"xxHEL"), (fr.NEW | fr.HOLE, b"LOyy")]     # a hole: two runs
    assert pieces[6] == [(fr.NEW, b"xHELLOy")]                                 # a hole filled in the same call
    assert pieces[11][0] == (fr.NEW, b"xxxxxxxHEL") and pieces[11][1][0] == fr.NEW | fr.HOLE   # a snapped frame
    second = {int(u["flow"]): (int(u["flags"]), got[1][0][int(u["at"]):int(u["at"] + u["len"])]) for u in got[1][1]}
    assert second[7] == (0, b"HELLO")          # the filler was late and is dropped; the stream goes on at next = 7
    assert second[8] == (0, b"LLOzz")          # a segment straddling next: the run continues exactly there
    assert second[12] == (0, b"HELLO")


def test_a_64_position_pattern_whose_tail_spans_many_tiny_segments():
    blob, _ = abi.flow_stream_compile(rc.LONG)
    calls, cap = rc.long_pattern()
    _, got = chain_follow(calls, cap, blob)
    s = b"__" + rc.LONG.encode() + b"__" + rc.LONG.encode()[:63] + b"!"
    assert got[0][0] == s and len(got[0][1]) == 1 and int(got[0][1][0]["flags"]) == fr.NEW


def per_stream(got):
    """{(flow, dir): [(call, flags, pos, bytes)]} over all calls."""
    out = {}
    for k, (wbytes, wruns, _, _) in enumerate(got):
        for u in wruns:
            key = (int(u["flow"]), int(u["flags"]) & 1)
            out.setdefault(key, []).append((k, int(u["flags"]), int(u["pos"]), wbytes[int(u["at"]):int(u["at"] + u["len"])]))
    return out


@pytest.mark.parametrize("seed", range(12))
def test_clean_captures_give_the_true_streams(seed):
    blob, _ = abi.flow_stream_compile(rc.PATTERN)
    calls, truth = rc.random_calls(seed, nflows=3, nbytes=500 + 97 * seed, ncalls=1 + seed % 3, clean=True)
    _, got = chain_follow(calls, 3, blob)
    streams = per_stream(got)
    assert set(streams) == set(truth)
    for key, s in truth.items():
        runs = streams[key]
        assert b"".join(r[3] for r in runs) == s, key
        assert not any(r[1] & fr.HOLE for r in runs)
        assert len({r[0] for r in runs}) == len(runs), "more than one run of a direction in a call"
        assert runs[0][1] & fr.NEW and not any(r[1] & fr.NEW for r in runs[1:])


@pytest.mark.parametrize("seed", range(12))
def test_disturbed_captures_every_run_is_its_piece_of_the_true_stream(seed):
    blob, _ = abi.flow_stream_compile("GET|POST" if seed % 2 else rc.PATTERN)
    calls, truth = rc.random_calls(100 + seed, nflows=4, nbytes=700, ncalls=3, clean=False)
    _, got = chain_follow(calls, 4, blob)
    holes = 0
    for wbytes, wruns, res, fres in got:
        assert int(wruns["len"].sum()) == fres["total"] == res["stream_bytes"]
        keys = [(int(u["flow"]) << 1 | int(u["flags"]) & 1, int(u["pos"])) for u in wruns]
        assert keys == sorted(keys) and len(set(keys)) == len(keys)
        assert list(wruns["at"]) == sorted(wruns["at"])
        for u in wruns:
            key = (int(u["flow"]), int(u["flags"]) & 1)
            first = [r for rows in calls for r in rows if r.key == key][0]
            t = int(u["pos"]) + first.off - 1
            assert wbytes[int(u["at"]):int(u["at"] + u["len"])] == truth[key][t:t + int(u["len"])], (key, int(u["pos"]))
            holes += bool(u["flags"] & fr.HOLE)
    assert holes >= 2


@pytest.mark.parametrize("which", ["query", "one", "short", "exact"])
def test_the_capacities_clip_the_outputs_and_nothing_else(which):
    blob, _ = abi.flow_stream_compile(rc.PATTERN)
    calls, _ = rc.random_calls(104, nflows=4, nbytes=700, ncalls=3, clean=False)
    caps = {"query": lambda t, r: (None, None), "one": lambda t, r: (1, 1), "short": lambda t, r: (t - 1, r - 1),
            "exact": lambda t, r: (t, r)}[which]
    _, clipped = chain_follow(calls, 4, blob, caps=caps)
    _, full = chain_follow(calls, 4, blob)
    for a, b in zip(clipped, full):
        assert a[3]["total"] == b[3]["total"] > 1 and a[3]["n_runs"] == b[3]["n_runs"] > 1
        assert a[1].tobytes() == b[1].tobytes()   # at and len are the true ones whatever the capacities


def test_without_a_pattern_the_bytes_are_the_same_and_nothing_is_matched():
    blob, _ = abi.flow_stream_compile(rc.PATTERN)
    calls, cap, _ = rc.crafted()
    with_model, with_pat = chain_follow(calls, cap, blob)
    plain_model, plain = chain_follow(calls, cap, None)
    assert sum(g[2]["hit_packets"] for g in with_pat) > 5
    for a, b in zip(with_pat, plain):
        assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[3] == b[3]
        assert b[2]["hit_packets"] == 0 and b[2]["new_hit_flows"] == 0
        assert {k: v for k, v in a[2].items() if k not in ("hit_packets", "new_hit_flows")} == \
               {k: v for k, v in b[2].items() if k not in ("hit_packets", "new_hit_flows")}
    wt, pt = with_model.table, plain_model.table
    assert (pt["d"]["d"] == 0).all() and (pt["d"]["hit_packets"] == 0).all() and (wt["d"]["d"] != 0).any()
    for name in rr.DIR_REC.names:
        if name not in ("d", "hit_packets"):
            assert (wt["d"][name] == pt["d"][name]).all(), name


@pytest.mark.parametrize("alias", ["hit", "rest"])
def test_hit_and_rest_in_place_of_select(alias):
    blob, _ = abi.flow_stream_compile(rc.PATTERN)
    calls, cap, _ = rc.crafted()
    chain_follow(calls, cap, blob, alias=alias)


def test_refusals_need_no_gpu():
    """Every refusal is decided before the context is looked at, each by its own reason, the null context last."""
    L = abi.lib()
    blob, _ = abi.flow_stream_compile(rc.PATTERN)
    data = (ctypes.c_uint8 * 256)()
    desc = (ctypes.c_uint64 * 4)()
    ids = (ctypes.c_uint32 * 4)()
    table = (ctypes.c_uint64 * 64)()
    res = (ctypes.c_uint64 * 8)()
    fres = (ctypes.c_uint64 * 4)()
    words = (ctypes.c_uint64 * 2)()
    more = (ctypes.c_uint64 * 2)()
    offs = (ctypes.c_int64 * 4)()
    outb = (ctypes.c_uint8 * 512)()
    runs = (ctypes.c_uint64 * 16)()
    places = (ctypes.c_uint64 * 4)()
    raw = (ctypes.c_uint8 * (1 << 17))()
    ip, tp, rp, fp, wp, mp, op, bp, ob, up, lp = (ctypes.addressof(x) for x in (ids, table, res, fres, words, more, offs, data, outb, runs, places))
    pp = blob.ctypes.data
    sp = (ctypes.addressof(raw) + 255) & ~255
    need = abi.flow_follow_scratch_bytes(2, 4)
    assert abi.flow_reasm_scratch_bytes(2, 4) < need <= (1 << 17) - 256
    out = abi.FlowReasmOut(wp, mp, rp, (ctypes.c_uint64 * 2)(0, 0))

    def said(rc_, word, code=BT_E_INVALID_ARGUMENT):
        msg = L.bt_last_error().decode()
        assert rc_ == code and word in msg, (word, rc_, msg)

    def good():
        return abi.Batch(ctypes.addressof(data), ctypes.addressof(desc), 0, 2, 256, abi.DESC_PACKED, 0)

    def fo_of(bytes_=ob, cap=512, runs_=up, run_cap=4, reserved0=0, place=lp, result=fp, reserved=(0, 0)):
        return abi.FlowFollowOut(bytes_, cap, runs_, run_cap, reserved0, place, result, (ctypes.c_uint64 * 2)(*reserved))

    def dev(word, frames=None, fo=fo_of(), pat=pp, pdev=bp, pbytes=len(blob), scratch=sp, nbytes=need, o=out, off=op):
        frames = good() if frames is None else frames
        said(L.bt_flow_follow_device(None, ctypes.byref(frames), ip, wp, off, 0, pat, pdev, pbytes, tp, 4, scratch, nbytes,
                                     ctypes.byref(o) if o is not None else None, ctypes.byref(fo) if fo is not None else None, None), word)

    dev("bt_flow_follow_device: null context")
    dev("null context", pat=None, pdev=None, pbytes=0)              # the plain follow
    dev("null context", fo=fo_of(bytes_=None, cap=0, runs_=None, run_cap=0, place=None))   # a size query
    dev("null out", o=None)                                          # what bt_flow_reasm_device refuses
    dev("null off", off=None)
    dev("scratch is not 256-byte aligned", scratch=sp + 8)
    dev("scratch_bytes", nbytes=need - 1)
    dev("scratch_bytes", nbytes=abi.flow_reasm_scratch_bytes(2, 4))
    dev("null fo", fo=None)
    dev("null fo->result", fo=fo_of(result=None))
    dev("null bytes with cap != 0", fo=fo_of(bytes_=None))
    dev("null runs with run_cap != 0", fo=fo_of(runs_=None))
    dev("runs is not 8-byte aligned", fo=fo_of(runs_=up + 4))
    dev("place is not 8-byte aligned", fo=fo_of(place=lp + 4))
    dev("fo->result is not 8-byte aligned", fo=fo_of(result=fp + 4))
    dev("reserved is not 0", fo=fo_of(reserved0=1))
    for k in range(2):
        dev("reserved is not 0", fo=fo_of(reserved=[int(j == k) for j in range(2)]))
    dev("overlaps the frames' buffer", fo=fo_of(bytes_=bp + 255, cap=1))
    dev("overlaps the frames' buffer", fo=fo_of(bytes_=bp - 8, cap=9))
    dev("null context", fo=fo_of(bytes_=bp + 256, cap=8))            # behind the buffer: no overlap
    dev("null pattern with a pattern_device", pat=None)
    dev("null pattern_device with a pattern", pdev=None)
    dev("pattern_bytes != 0 without a pattern", pat=None, pdev=None)
    dev("pattern_bytes below a blob's header", pbytes=0)             # the pattern's own check comes first
    f = good()
    f.n = 0
    dev("null context", frames=f, scratch=None, nbytes=0)            # an empty batch needs no scratch

    def host(word, fo=fo_of(), pat=pp, pbytes=len(blob), o=out, d=ctypes.addressof(desc)):
        said(L.bt_flow_follow_host(bp, 256, d, 2, ip, wp, op, 0, pat, pbytes, tp, 4, ctypes.byref(o) if o is not None else None,
                                   ctypes.byref(fo) if fo is not None else None), word)

    host("bt_flow_follow_host: null base / desc", d=None)
    host("null out", o=None)
    host("null fo", fo=None)
    host("null fo->result", fo=fo_of(result=None))
    host("null bytes with cap != 0", fo=fo_of(bytes_=None))
    host("null runs with run_cap != 0", fo=fo_of(runs_=None))
    host("place is not 8-byte aligned", fo=fo_of(place=lp + 2))
    host("reserved is not 0", fo=fo_of(reserved=(0, 9)))
    host("overlaps the frames' buffer", fo=fo_of(bytes_=bp + 100, cap=4))
    host("pattern_bytes != 0 without a pattern", pat=None)
    host("a pattern with pattern_bytes == 0", pbytes=0)


def test_an_empty_batch_writes_both_results_and_nothing_else():
    blob, _ = abi.flow_stream_compile(rc.PATTERN)
    tab = np.zeros(2, abi.FlowReasmRec)
    for pat in (blob, None):
        out, runs = np.full(8, POISON, np.uint8), np.frombuffer(bytes([POISON]) * 64, abi.FlowFollowRun).copy()
        res, fres = abi.flow_follow_host(np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32), None, None, BIDIR, pat, tab,
                                         out_bytes=out, runs=runs)
        assert result_of(res) == {k: 0 for k in rr.RESULT} and follow_result_of(fres) == {k: 0 for k in fr.FRESULT}
        assert not tab.tobytes().strip(b"\0") and (out == POISON).all() and runs.tobytes() == bytes([POISON]) * 64


def test_flowfollow_host_check_builds_and_passes(tmp_path):
    """tools/flowfollow_host_check.cpp: the argument checks and the chain of the two host forms against an oracle on
    true 64-bit positions, under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program."""
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "flowfollow_host_check")
    # the sanitizer runtimes linked into the program: it runs the same whatever else a process preloads
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",
                    "-I" + os.path.join(root, "include"), "-I" + os.path.join(root, "beatrice_amd", "csrc"),
                    os.path.join(root, "tools", "flowfollow_host_check.cpp"), os.path.join(root, "beatrice_amd", "csrc", "bt_regex_dfa.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all checks hold" in r.stdout, r.stdout + r.stderr
