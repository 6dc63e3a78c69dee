"""CPU: the extended PAYLOAD subset (BT_DFA_EXTENDED; beatrice_amd/csrc/bt_regex_dfa.cpp) —
\\b and \\B, POSIX bracket classes and DFAs of more than 254 live states (the wide blob) —
checked without a GPU: the default entry classifies and compiles exactly as before, the
flag adds coverage only, and the host executor of every new blob decides the recorded
frames of tests/golden/regex_ext.* (made by make_regex_ext.py from the compiled reference)
as the reference's std::regex did."""
import ast
import json
import os
import re
import time

import numpy as np
import pytest

import oracle_lib as ol
from beatrice_amd import abi, synth
from conftest import GOLDEN, load_golden

ON_HOST = ["\\bfoo", "(ab)\\1", "(?=a)b", "[[:alpha:]]", "\\cA", "\\u0041", "\\a", "(a|b)*a(a|b){12}"]
STILL_HOST = ["(ab)\\1", "(?=a)b", "\\cA", "\\u0041", "\\a", "(a|b)*a(a|b){12}", "[[.a.]]", "[[=a=]]"]
SUPPORTED = ["GET", "GET|POST", "^GET /", "HTTP/1\\.[01]", "[^]", "[]", "^$", "a|", "x{0}y", "\\0", "(?:a|b)*c",
             "[\\x80-\\xff]{4,}", "\\s+$", "a**", "a{2,3}?"]
WIDE_TAG = b"\xfe\xff"
POOL = 16384


@pytest.fixture(scope="module")
def fixture():
    z = np.load(os.path.join(GOLDEN, "regex_ext.npz"), allow_pickle=False)
    with open(os.path.join(GOLDEN, "regex_ext.json")) as fh:
        meta = json.load(fh)
    g = {k: z[k] for k in z.files}
    off, ln = synth.desc_off(g["desc"]), synth.desc_len(g["desc"])
    g["frames"] = [bytes(g["data"][int(o):int(o) + int(n)]) for o, n in zip(off, ln)]
    return g, meta


def test_default_classification_unchanged():
    for e in ON_HOST:
        assert abi.payload_dfa(e) is None, e
        for fl in (abi.DFA_NO_PAIRS, abi.DFA_NO_BITPAR, abi.DFA_NO_BITPAR | abi.DFA_NO_PAIRS):
            assert abi.payload_dfa(e, fl) is None, (e, fl)


def test_extended_classification():
    for e in STILL_HOST:
        assert abi.payload_dfa(e, abi.DFA_EXTENDED) is None, e
    for e in ("\\bfoo", "[[:alpha:]]", "\\B", "[^[:alnum:]_]", "(a|b)*a(a|b){8}"):
        assert abi.payload_dfa(e, abi.DFA_EXTENDED) is not None, e
    for e in ("[[:word:]]", "\\b*", "[a-[:digit:]]", "["):   # std::regex rejects these itself
        with pytest.raises(abi.BtError):
            abi.payload_dfa(e, abi.DFA_EXTENDED)
    # \b \B never take the bit-parallel form; a POSIX class is a byte set and may
    assert abi.payload_dfa("\\bGET", abi.DFA_EXTENDED)[:2] != b"\xff\xff"
    assert abi.payload_dfa("[[:digit:]]{3}", abi.DFA_EXTENDED)[:2] == b"\xff\xff"


def test_supported_blobs_identical_with_flag():
    assert len(SUPPORTED) == 15
    for e in SUPPORTED:
        for base in (0, abi.DFA_NO_PAIRS, abi.DFA_NO_BITPAR, abi.DFA_NO_BITPAR | abi.DFA_NO_PAIRS):
            a, b = abi.payload_dfa(e, base), abi.payload_dfa(e, base | abi.DFA_EXTENDED)
            assert a is not None and a == b, (e, base)


def test_posix_classes_are_c_locale_byte_sets(fixture):
    """The 256 one-byte windows at the fixture's end against every class name."""
    g, meta = fixture
    n = len(g["frames"])
    for name in meta["classes"]:
        p = meta["patterns"].index(f"[[:{name}:]]")
        blob = abi.payload_dfa(f"[[:{name}:]]", abi.DFA_EXTENDED)
        got = [b for b in range(256) if abi.payload_dfa_search(blob, bytes([b]))]
        want = [b for b in range(256) if g["code"][p, n - 256 + b] == 0]
        assert got == want, name
        assert want and max(want) < 0x80, name
    w = meta["patterns"].index("[[:w:]]")
    assert int((g["code"][w, n - 256:] == 0).sum()) == 63


def test_fixture_patterns_match_reference(fixture):
    g, meta = fixture
    assert len(meta["patterns"]) >= 35 and len(g["frames"]) >= 1500
    for p, expr in enumerate(meta["patterns"]):
        assert abi.payload_dfa(expr) is None, f"/{expr}/ is in the default subset: not a test of the extension"
        for fl in (abi.DFA_EXTENDED, abi.DFA_EXTENDED | abi.DFA_NO_BITPAR | abi.DFA_NO_PAIRS):
            blob = abi.payload_dfa(expr, fl)
            assert blob is not None, f"/{expr}/ stays on the host under DFA_EXTENDED"
            got = np.array([abi.payload_dfa_eval(blob, f) for f in g["frames"]])
            bad = np.nonzero(got != (g["code"][p] == 0))[0]
            assert len(bad) == 0, f"/{expr}/ flags {fl}: {len(bad)} frames differ from the reference: {bad[:20].tolist()}"


def test_wide_form(fixture):
    _, meta = fixture
    for expr in meta["wide"]:
        blob = abi.payload_dfa(expr, abi.DFA_EXTENDED)
        assert blob[:2] == WIDE_TAG, expr
        C, K, init = (int.from_bytes(blob[o:o + 2], "little") for o in (2, 4, 6))
        assert 254 < K <= 4096 and 2 <= C <= 256 and init <= K + 1
        assert len(blob) == 12 + 256 + (K + 3) // 4 * 4 + 2 * K * C
        assert len(blob) < POOL
        nxt = np.frombuffer(blob[len(blob) - 2 * K * C:], np.uint16)
        assert nxt.max() <= K + 1   # every entry a live state or a sink
    # a narrow DFA keeps the narrow layout even when the subset construction needed the room
    assert abi.payload_dfa("(ab)*c.{6}d") is None
    assert abi.payload_dfa("(ab)*c.{6}d", abi.DFA_EXTENDED)[:2] not in (WIDE_TAG, b"\xff\xff")
    # the wide table that no pool holds
    assert abi.payload_dfa("(a|b)*a(a|b){12}", abi.DFA_EXTENDED) is None


class Gen:
    """Random patterns over the extended grammar."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)

    def r(self, n):
        return int(self.rng.integers(n))

    def atom(self, depth):
        k = self.r(10)
        if k == 0 and depth < 2:
            return "(" + self.seq(depth + 1) + "|" + self.seq(depth + 1) + ")"
        if k == 1 and depth < 2:
            return "(?:" + self.seq(depth + 1) + ")"
        if k == 2:
            names = ["alpha", "digit", "alnum", "upper", "lower", "space", "blank", "punct", "print", "graph",
                     "cntrl", "xdigit", "d", "w", "s"]
            s = "[" + ("^" if self.r(2) else "") + f"[:{names[self.r(15)]}:]"
            s += "_" if self.r(2) else ""
            s += f"[:{names[self.r(15)]}:]" if self.r(3) == 0 else ""
            return s + "]"
        return [".", "\\w", "\\d", " ", "a", "b", "_", "1", "G", "-"][self.r(10)]

    def seq(self, depth=0):
        s, n = "", 1 + self.r(4)
        for i in range(n):
            k = self.r(12)
            if k == 0:
                s += "\\b"
            elif k == 1:
                s += "\\B"
            elif k == 2 and i == 0:
                s += "^"
            elif k == 3 and i == n - 1:
                s += "$"
            else:
                a = self.atom(depth)
                # no * + on a group: std::regex backtracks without bound on (x*)* and its like
                q = ["?", "{2}", "", "", ""] if a[0] == "(" else ["*", "+", "?", "{2}", "{1,3}", "", "", "", "", ""]
                s += a + q[self.r(len(q))]
        return s


@pytest.mark.skipif(not ol.ref_available(), reason="oracle/_ref (compiled reference) not built")
def test_random_sweep_against_reference(fixture):
    g, _ = fixture
    seed = int(time.time()) & 0xFFFFFF
    print(f"seed {seed}")
    gen = Gen(seed)
    idx = np.random.default_rng(seed).choice(len(g["frames"]), 300, replace=False)
    frames = [g["frames"][i] for i in idx]
    data, desc = synth.pack_frames(frames, align=1)
    t0, taken, tried = time.time(), 0, 0
    while time.time() - t0 < 8.0 and tried < 400:
        expr = gen.seq()
        tried += 1
        try:
            blob = abi.payload_dfa(expr, abi.DFA_EXTENDED)
        except abi.BtError:
            continue
        if blob is None:
            continue
        code, _ = ol.ref_filter(data, desc, len(frames), [{"type": abi.PAYLOAD, "expr": expr, "priority": 1}])
        got = np.array([abi.payload_dfa_eval(blob, f) for f in frames])
        bad = np.nonzero(got != (code == 0))[0]
        assert len(bad) == 0, f"seed {seed} /{expr}/: frames {idx[bad][:20].tolist()} differ from the reference"
        taken += 1
    print(f"{taken} of {tried} random patterns compiled and agreed")
    assert taken >= 20


def _survey_patterns():
    _, man = load_golden("edge")
    exprs = {f["expr"] for fs in man["filter_sets"].values() for f in fs if f["type"] == abi.PAYLOAD and f.get("expr")}
    with open(os.path.join(os.path.dirname(GOLDEN), "cpp", "test_regex_dfa.cpp")) as fh:
        m = re.search(r"const char\* fixed\[\] = \{(.*?)\};", fh.read(), re.S)
    exprs |= {ast.literal_eval(s) for s in re.findall(r'"(?:[^"\\]|\\.)*"', m.group(1))}
    return sorted(exprs)


def test_host_fallback_share():
    """Of the PAYLOAD expressions in the golden manifest and the C++ fuzzer's fixed list that
    std::regex accepts: how many stay on the host, without the flag and with it."""
    host = {0: [], abi.DFA_EXTENDED: []}
    valid = 0
    for e in _survey_patterns():
        try:
            for fl in host:
                if abi.payload_dfa(e, fl) is None:
                    host[fl].append(e)
            valid += 1
        except abi.BtError:
            pass
    a, b = len(host[0]), len(host[abi.DFA_EXTENDED])
    print(f"host fallback: {a} of {valid} patterns ({100 * a / valid:.1f} %) by default, "
          f"{b} of {valid} ({100 * b / valid:.1f} %) with DFA_EXTENDED; left: {host[abi.DFA_EXTENDED]}")
    assert set(host[abi.DFA_EXTENDED]) <= set(host[0])
    assert {"\\bfoo", "[[:alpha:]]"} <= set(host[0]) - set(host[abi.DFA_EXTENDED])
