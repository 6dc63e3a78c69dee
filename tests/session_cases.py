"""Traffic that lives, dies and comes back, for the session model's tests (test_session_model.py,
test_gpu_session.py): a deterministic generator of conversations with a scheduled life, the scenarios
as lists of operations (a batch through the whole chain, an expire with its side moves, a checkpoint),
the model's run over a scenario, and the one comparison both drivers use: what a driver observed
against what session_ref.SessionModel expects, exactly, naming the table, the key and its life."""
import functools

import numpy as np

import flow_ref as fr
import flowmark_ref as mr
import flowseq_ref as qr
import flowtab_ref as ftr
import flowtcp_ref as tr
import session_ref as sm
from flowstat_cases import ip4, tcp_hdr

S, K, P, F, R = tr.SYN, tr.ACK, tr.PSH, tr.FIN, tr.RST
KINDS = ("tcp", "tcp_big", "udp", "icmp", "tcp6", "udp6", "tag_tcp", "qinq_udp", "tag_tcp6", "fragment")
UNKEYED = [bytes(12) + b"\x08\x06" + bytes(28),                                                      # ARP
           bytes(10),                                                                                # a runt
           bytes(12) + b"\x81\x00\x00\x01\x81\x00\x00\x02\x81\x00\x00\x03\x08\x00" + bytes(40)]       # three tags
LIMITS = [(0, 0), (3, 0), (0, 2000), (5, 4000)]
PAYLOADS = (0, 0, 24, 200, 700)
KEY_BYTES = {fr.NONE: 0, fr.V4: 8, fr.V4_L4: 12, fr.V6: 32, fr.V6_L4: 36}


def ip6(nh, l4, src, dst, hop=64, vlan=0):
    tag = b"".join((b"\x88\xa8" if k == 0 and vlan == 2 else b"\x81\x00") + b"\x00\x07" for k in range(vlan))
    return bytes(12) + tag + b"\x86\xdd" + b"\x60\x00\x00\x00" + len(l4).to_bytes(2, "big") + bytes([nh, hop]) + bytes(src) + bytes(dst) + l4


def udp_hdr(sp, dp, payload):
    return sp.to_bytes(2, "big") + dp.to_bytes(2, "big") + (8 + payload).to_bytes(2, "big") + bytes(2) + bytes(payload)


class Conversation:
    """Two endpoints and a kind. a is the smaller endpoint as a byte string; a tcp_big conversation is
    opened by b. frame(step, ...) gives its step-th packet of a window: a handshake first, then data both ways."""

    def __init__(self, k, kind, servers):
        self.k, self.kind = k, kind
        self.v6 = kind in ("tcp6", "udp6", "tag_tcp6")
        lo, hi = [10, KINDS.index(kind), k >> 8, k & 255], [172, 16, 0, k % servers]
        if self.v6:
            lo, hi = [0x20, 1, 0xd, 0xb8] + [0] * 8 + lo, [0x20, 1, 0xd, 0xb8] + [0xff] * 8 + hi
        self.addr = (lo, hi)
        self.ports = (1024 + k, (443, 80, 8080)[k % 3])
        self.vlan = {"tag_tcp": 1, "qinq_udp": 2, "tag_tcp6": 1}.get(kind, 0)
        self.opener = 1 if kind == "tcp_big" else 0
        self.tcp = "tcp" in kind
        self.ttl = (64 - k % 5, 128 - k % 7)

    def wrap(self, d, proto, l4, flags=0):
        src, dst = self.addr[d], self.addr[1 - d]
        if self.v6:
            return ip6({1: 58}.get(proto, proto), l4, src, dst, self.ttl[d], self.vlan)
        return ip4(proto, l4, src, dst, ttl=self.ttl[d], flags=flags, vlan=self.vlan)

    def frame(self, step, closing, pay):
        """closing: 0, or how this packet ends the connection (1: FIN from the opener, 2: FIN back, 3: RST)."""
        d = (self.opener + step) % 2 if step < 2 or step % 3 else self.opener
        sp, dp = (self.ports if d == 0 else self.ports[::-1])
        if self.tcp:
            if closing:
                d = self.opener if closing != 2 else 1 - self.opener
                sp, dp = (self.ports if d == 0 else self.ports[::-1])
                return self.wrap(d, 6, tcp_hdr(sp, dp, (F | K, F | K, R)[closing - 1]))
            fl = (S, S | K, K)[step] if step < 3 else K | P
            return self.wrap(d, 6, tcp_hdr(sp, dp, fl) + bytes(pay if step >= 3 else 0))
        if "udp" in self.kind:
            return self.wrap(d, 17, udp_hdr(sp, dp, pay))
        if self.kind == "icmp":
            return self.wrap(d, 1, bytes([8 if d == 0 else 0]) + bytes(7) + bytes(pay))
        return self.wrap(d, 6, tcp_hdr(sp, dp, K) + bytes(8), flags=0x2000)   # a fragment: the key is the addresses alone


def make_conversations(count, kinds=KINDS, servers=7):
    return [Conversation(k, kinds[k % len(kinds)], servers) for k in range(count)]


def draw_batch(rng, convs, active, weights, n, base, span, steps, closers=()):
    """n packets of the active conversations, interleaved at random (each conversation's own packets in its
    script order), stamped at random inside [base, base + span): not monotonic. At least one unkeyed frame
    when n >= 2. steps: conversation -> packets of its window so far (kept by the caller)."""
    if n == 0:
        return [], np.zeros(0, np.uint64)
    who = rng.choice(len(active), size=n, p=np.asarray(weights, float) / np.sum(weights))
    unkeyed = rng.random(n) < 0.03
    if n >= 2:
        unkeyed[int(rng.integers(0, n))] = True
    left = np.bincount(who[~unkeyed], minlength=len(active))
    frames = []
    for i in range(n):
        if unkeyed[i]:
            frames.append(UNKEYED[int(rng.integers(0, len(UNKEYED)))])
            continue
        c = convs[active[who[i]]]
        left[who[i]] -= 1
        closing = 0
        if c.k in closers and c.tcp and left[who[i]] < 2 and steps.get(c.k, 0) >= 3:
            closing = 3 if c.k % 4 == 0 else 2 - left[who[i]]
        frames.append(c.frame(steps.get(c.k, 0), closing, PAYLOADS[int(rng.integers(0, len(PAYLOADS)))]))
        steps[c.k] = steps.get(c.k, 0) + 1
    return frames, (base + rng.integers(0, span, n)).astype(np.uint64)


def is_hit(frame):
    """The verdict stand-in, from the frame's bytes alone: TCP to port 443."""
    kb, klass = fr.walk(frame)
    return klass in (fr.V4_L4, fr.V6_L4) and tr.tcp_of_frame(frame)[0] and kb[-2:] == (443).to_bytes(2, "big")


def batch_op(rng, b, frames, ts, everyone=False):
    """The chain's parameters for batch b: the selection, the hits, the mark, the limits, the select op all rotate."""
    n = len(frames)
    select = None if everyone or b % 3 == 0 else rng.random(n) < 0.9
    cache = {}
    for f in frames:
        if f not in cache:
            cache[f] = is_hit(f)
    hit = np.array([cache[f] for f in frames], bool)
    hit |= rng.random(n) < 0.02   # and a few others, unkeyed and unselected packets among them
    mp, mb = LIMITS[b % len(LIMITS)]
    return {"op": "batch", "frames": frames, "ts": ts, "select": select, "hit": hit, "mark": 1 << (b % 3), "mp": mp, "mb": mb,
            "seq_flags": qr.KEEP_UNKEYED if b % 2 else 0, "sel_op": (mr.SET, mr.AND, mr.OR, mr.ANDNOT)[b % 4],
            "sel_mask": (1, 3, 2, 5)[b % 4], "sel_flags": mr.ALL_BITS if b % 4 == 1 else 0}


class Scenario:
    def __init__(self, name, flags, flow_cap, slots, ops, k=16, want=()):
        self.name, self.flags, self.flow_cap, self.slots, self.ops, self.k, self.want = name, flags, flow_cap, slots, ops, k, want
        self.host_cap = 2 * flow_cap


def expire_op(now, idle, closed_idle=None, cap=None):
    return {"op": "expire", "now": now, "idle": idle, "closed_idle": closed_idle, "cap": cap}


CHECK = {"op": "check"}
T = 10_000   # a batch's stamps lie in [T b, T b + T / 2)


def staged(seed, count, sizes, plan, expires, kinds=KINDS, everyone=False):
    """Batches of the given sizes. plan[b]: for each third of the conversations (by k % 3), the share of it that is
    active in batch b; a conversation that stops being active closes its connection. expires: after batch b."""
    rng = np.random.default_rng(seed)
    convs = make_conversations(count, kinds)
    on = [[k for k in range(count) if rng.random() < plan[b][k % 3]] for b in range(len(sizes))]
    ops, steps = [], {}
    for b, n in enumerate(sizes):
        active = on[b] or [0]
        after = set(on[b + 1]) if b + 1 < len(sizes) else set()
        for k in active:
            if b == 0 or k not in on[b - 1]:
                steps[k] = 0   # a new window: the handshake again
        weights = [30.0 if k % 53 == 0 else 1.0 for k in active]   # a few heavy conversations
        frames, ts = draw_batch(rng, convs, active, weights, n, T * b, T // 2, steps, closers={k for k in active if k not in after})
        ops.append(batch_op(rng, b, frames, ts, everyone))
        for e in expires.get(b, ()):
            ops += [e, CHECK]
    ops.append(CHECK)
    return ops


@functools.lru_cache(maxsize=None)
def scenario(name):
    B = ftr.BIDIRECTIONAL
    if name in ("churn", "xdp"):
        # the first third talks early, goes quiet and returns; the second arrives with the large batches; the third is always there
        plan = [(.5, 0, .3), (.5, 0, .3), (.6, 0, .3), (.1, 0, .1), (0, 0, 0), (.1, 1, .6), (.5, .9, .6), (1, 1, 1)]
        exp = {3: [expire_op(3 * T + T, 2 * T + T // 2, cap=600)],                 # what batch 0 alone saw leaves
               5: [expire_op(5 * T + T, T + T // 2, cap=20)],                      # more idle flows than room: truncated
               6: [expire_op(6 * T + T, T + T // 2, cap=4096)]}                    # the rest of them, and batch 5's quiet ones
        ops = staged(11, 600, [63, 64, 65, 1, 0, 4097, 16385, 4096], plan, exp)
        if name == "xdp":
            ops = [o for o in ops[:ops.index(exp[3][0])] if o["op"] == "batch"] + [CHECK]
            return Scenario("xdp", B, 4096, 0, ops)
        return Scenario("churn", B, 4096, 0, ops, want=("returned", "truncated", "most_in_a_batch"))
    if name == "full":
        # 257 flows at 257 slots... the layout's minimum is max(128, flow_cap) rounded up to a power of two
        plan = [(1, .6, .6), (.3, 1, .6), (.2, .3, 1), (1, 1, 1), (.5, .5, .5)]
        exp = {0: [expire_op(T, T, cap=300)],                                       # nothing is idle yet
               1: [expire_op(T + T, T + T // 4, cap=100)],
               2: [expire_op(2 * T + T, T + T // 4, cap=60)],                       # truncated
               3: [expire_op(3 * T + T, T // 4, cap=257)]}
        ops = staged(23, 450, [1500, 900, 1100, 1300, 800], plan, exp)
        return Scenario("full", B, 257, 512, ops, k=300, want=("returned", "truncated", "admitted_after_overflow"))
    if name == "closed":
        plan = [(1, .5, .2), (.5, 1, .5), (.2, .5, 1), (1, .2, .5), (.6, .6, .6)]
        exp = {0: [expire_op(T, 3 * T, closed_idle=T // 4, cap=10)],            # closed connections only, truncated
               1: [expire_op(T + T, T + T // 4, cap=400)],                          # plain: the TCP table by the generic move
               2: [expire_op(2 * T + T, 3 * T, closed_idle=T // 2, cap=400)],
               3: [expire_op(3 * T + T, T + T // 4, cap=400), expire_op(3 * T + T, 3 * T, closed_idle=0, cap=400)]}
        ops = staged(37, 240, [1000, 1500, 2000, 1500, 1000], plan, exp, kinds=("tcp", "tcp_big", "tcp6", "tag_tcp", "udp", "tag_tcp6"))
        return Scenario("closed", B, 1024, 0, ops, want=("returned", "truncated"))
    assert name.startswith("l3")
    # L3_ONLY: one key per address pair, many packets per flow per batch: long segments of the sorted list
    flags, cap = {"l3_1": (ftr.L3_ONLY, 1), "l3_64": (ftr.L3_ONLY | B, 64), "l3_64u": (ftr.L3_ONLY, 64)}[name]
    plan = [(1, 1, 0), (1, 0, 0), (1, 1, 1), (0, 1, 1)]
    exp = {0: [expire_op(T, T, cap=64)],                                            # removes nothing
           1: [expire_op(T + T, T + T // 4, cap=5)],                                # truncated
           2: [expire_op(2 * T + T, 0, cap=None)]}                                  # expired == NULL: everything goes
    ops = staged(41, 36, [3000, 1000, 20000, 2000], plan, exp, kinds=("tcp", "udp", "tcp6", "icmp", "tag_tcp"), everyone=True)
    want = ("most_in_a_batch", "expired_nothing", "expired_all") + (("returned", "truncated", "spans_a_chunk") if cap == 64 else ("admitted_after_overflow",))
    return Scenario(name, flags, cap, 0, ops, k=8, want=want)


SCENARIOS = ["churn", "full", "closed", "l3_1", "l3_64", "l3_64u"]


@functools.lru_cache(maxsize=None)
def expected(name):
    """The model's run over a scenario: (the model, what each operation must give)."""
    scn = scenario(name)
    model = sm.SessionModel(scn.flags, scn.flow_cap, scn.slots)
    out = []
    for o in scn.ops:
        if o["op"] == "batch":
            out.append(model.update(o["frames"], o["ts"], o["select"], o["hit"], o["mark"], o["mp"], o["mb"], o["seq_flags"],
                                    o["sel_op"], o["sel_mask"], o["sel_flags"]))
        elif o["op"] == "expire":
            out.append(model.expire(o["now"], o["idle"], o["closed_idle"], o["cap"]))
        else:
            out.append(model.checkpoint(scn.k, scn.host_cap))
    return model, out


def assert_not_vacuous(name):
    """Conditions on the inputs, on the model alone: the scenario meets what it is there for."""
    scn = scenario(name)
    st = expected(name)[0].stats
    for what in scn.want:
        assert st[what] > (64 if what == "most_in_a_batch" else 0), f"{name}: vacuous, {what} = {st[what]}"
    for o in scn.ops:
        if o["op"] == "batch" and len(o["frames"]) >= 2:
            assert any(fr.walk(f)[1] == fr.NONE for f in o["frames"]), f"{name}: a batch without an unkeyed frame"
    if name == "full":
        over = [e["track"]["overflow_packets"] for o, e in zip(scn.ops, expected(name)[1]) if o["op"] == "batch"]
        assert all(v > 0 for v in over[:2]), f"full: no overflow in a batch before an expire made room: {over}"


def pack(frames):
    """(data, packed descriptors): the frames back to back with gaps of 0 .. 4 bytes, so that they start at every alignment."""
    parts, desc, at = [], np.zeros(len(frames), np.uint64), 0
    for i, f in enumerate(frames):
        gap = i % 5
        parts.append(bytes(gap) + f)
        desc[i] = (at + gap) | len(f) << 48
        at += gap + len(f)
    data = np.frombuffer(b"".join(parts) + bytes(8), np.uint8)
    return data, desc


def words(bits, rng=None):
    """Verdict-layout words of a bool array; with rng, garbage in the last word's bits at or above n (must be ignored)."""
    w = fr.pack_bits(np.asarray(bits, bool)).copy()
    n = len(bits)
    if rng is not None and n % 64:
        w[-1] |= np.uint64(int(rng.integers(0, 1 << 62)) << (n % 64) & sm.U64)
    return w


# ---- the comparison: what a driver observed against the model, exactly

def _key(key, life=None):
    klass, kb = key
    return f"key class {klass} {kb.hex()}" + ("" if life is None else f" life {life}")


def _same_dict(where, got, want):
    assert got == want, f"{where}: " + ", ".join(f"{k} = {got.get(k)} != {want[k]}" for k in want if got.get(k) != want[k])


def _same_rows(where, got, want, keys, lives=None):
    """Two record arrays, row by row; the first row that differs is named by its key."""
    assert len(got) == len(want), f"{where}: {len(got)} records, not {len(want)}"
    if len(want) == 0:
        return
    g, w = np.ascontiguousarray(got).view(np.uint8).reshape(len(want), -1), np.ascontiguousarray(want).view(np.uint8).reshape(len(want), -1)
    bad = np.nonzero((g != w).any(axis=1))[0]
    if len(bad):
        f = int(bad[0])
        who = _key(keys[f], lives[f] if lives else None) if f < len(keys) else "behind the live flows"
        fields = [n for n in want.dtype.names if want[f][n].tobytes() != np.ascontiguousarray(got).view(want.dtype)[f][n].tobytes()]
        raise AssertionError(f"{where}: record {f} ({who}) differs in {fields}: got {np.ascontiguousarray(got).view(want.dtype)[f]}, "
                             f"want {want[f]}; {len(bad)} records differ")


def compare(name, observed, where=""):
    """Every operation's observed outputs against the model's. observed[j] belongs to scenario(name).ops[j]."""
    scn = scenario(name)
    model, exp = expected(name)
    assert len(observed) == len(exp)
    ever_expired = np.zeros(2, np.int64)   # packets, bytes of every exported flow
    exported_all = True
    for j, (o, want, got) in enumerate(zip(scn.ops, exp, observed)):
        at = f"{where}{name} op {j} ({o['op']})"
        if o["op"] == "batch":
            n = want["n"]
            for field in ("flow_id", "seq", "byte_off"):
                bad = np.nonzero(got[field][:n] != want[field])[0]
                if len(bad):
                    i = int(bad[0])
                    raise AssertionError(f"{at}: {field}[{i}] = {got[field][i]} != {want[field][i]} ({_key(want['keys'][i])}); {len(bad)} differ")
            for field in ("seq_words", "msel_words"):
                bad = np.nonzero(got[field][:(n + 63) // 64] != want[field])[0]
                assert len(bad) == 0, f"{at}: {field} differs at words {bad[:8]}"
            for field in ("track", "tcp", "stat", "mark", "seq_res", "msel"):
                _same_dict(f"{at}: {field} result", got[field], want[field])
        elif o["op"] == "expire":
            if o["cap"] is not None:   # who left, by key, before any count: a wrong rule is named by the first key it misplaces
                left = [(int(r["klass"]), bytes(r["key"][:KEY_BYTES[int(r["klass"])]])) for r in got["track"]]
                for x, (g, w) in enumerate(zip(left + [None] * len(want["keys"]), want["keys"] + [None] * len(left))):
                    assert g == w, (f"{at}: table track, expired[{x}]: the call's is {_key(g) if g else 'nothing'}, the model's is "
                                    f"{_key(w, want['lives'][x]) if w else 'nothing'}")
            _same_dict(f"{at}: result", got["result"], want["result"])
            nb = want["result"]["n_flows_before"]
            bad = np.nonzero(got["remap"][:nb] != want["remap"])[0]
            assert len(bad) == 0, f"{at}: remap differs at old numbers {bad[:8]}: {got['remap'][bad[:8]]} != {want['remap'][bad[:8]]}"
            if o["cap"] is None:
                exported_all = exported_all and want["result"]["n_expired"] == 0
                continue
            for t in sm.TABLES:
                _same_rows(f"{at}: expired {t}", got[t], want[t], want["keys"], want["lives"])
            ever_expired += [int(got["track"]["packets"].sum()), int(got["track"]["bytes"].sum())]
        else:
            _same_dict(f"{at}: header", got["hdr"], want["hdr"])
            for t in sm.TABLES:   # the whole table: the live keys' records, zeros behind them
                _same_rows(f"{at}: table {t}", got[t], want[t], want["keys"], want["lives"])
            for m, w in want["top"].items():
                g = got["top"][m]
                _same_dict(f"{at}: top metric {m} result", g["result"], w["result"])
                assert [want["keys"][f] for f in g["ids"]] == w["keys"], f"{at}: top metric {m}: ids {g['ids']} are not the keys the model ranks first"
                assert (g["values"] == w["values"]).all(), f"{at}: top metric {m} values"
                _same_rows(f"{at}: top metric {m} records", g["recs"], w["recs"], w["keys"])
                _same_rows(f"{at}: top metric {m} tcp records", g["tcps"], w["tcps"], w["keys"])
            _same_dict(f"{at}: hosts result", got["hosts"]["result"], want["hosts"]["result"])
            bad = np.nonzero(got["hosts"]["endpoint_host"] != want["hosts"]["endpoint_host"])[0]
            assert len(bad) == 0, f"{at}: endpoint_host differs at {bad[:8]}"
            wh, gh = want["hosts"]["hosts"], got["hosts"]["hosts"]
            assert len(gh) == len(wh), f"{at}: {len(gh)} hosts, not {len(wh)}"
            for h in range(len(wh)):
                assert gh[h].tobytes() == wh[h].tobytes(), f"{at}: host {h} ({bytes(wh[h]['addr']).hex()}): got {gh[h]}, want {wh[h]}"
            # identities that need no model
            hdr, rec, nf = got["hdr"], got["track"], got["hdr"]["n_flows"]
            pk = rec["packets"].sum(axis=1)
            if exported_all:
                assert hdr["keyed_packets"] == int(pk.sum()) + int(ever_expired[0]) + hdr["overflow_packets"], f"{at}: packets are lost"
                assert hdr["keyed_bytes"] == int(rec["bytes"].sum()) + int(ever_expired[1]) + hdr["overflow_bytes"], f"{at}: bytes are lost"
            assert (got["seq"]["packets"] == pk).all(), f"{at}: a flow's numbered packets are not its packets"
            assert (got["mark"]["hit_packets"] <= pk).all() and (got["stat"]["payload_packets"].sum(axis=1) <= pk).all(), at
            assert not rec[nf:].tobytes().strip(b"\0"), f"{at}: records behind n_flows"
    return model


def same(a, b):
    """Deep bit-equality of two observations (dicts, lists, arrays, numbers)."""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.tobytes() == b.tobytes()
    return a == b
