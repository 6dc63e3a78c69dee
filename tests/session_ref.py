"""A model of the whole flow chain that never sees a flow number: the tracker, its four side tables
(TCP, statistics, marks, sequence), the expires and the read-only views, keyed by (class, canonical
key bytes). Only the admission rules of include/beatrice_gpu.h are restated here (who gets in, who
overflows, who is idle, who leaves and in which order); everything a table holds is derived per key
from that key's own packets, by the existing restatements applied with flow_id = zeros to a
one-record table. A key's flow number is its position among the live keys, nothing else. Nothing here
imports flowtrack_ref.Tracker, flowstat_ref.side_move or the code under test (dtypes and constants
only), so a mistake in their flow-number bookkeeping cannot cancel out."""
import numpy as np

import flow_ref as fr
import flowmark_ref as mr
import flowseq_ref as qr
import flowstat_ref as sr
import flowtab_ref as ftr
import flowtcp_ref as tr
from beatrice_amd.abi import FlowHostRec
from flowtrack_ref import EXPIRED, FLOW_TRACK_REC, MAGIC

U64 = (1 << 64) - 1
TABLES = ("track", "tcp", "stat", "mark", "seq")
SIDE = {"tcp": tr.TCP_REC, "stat": sr.STAT_REC, "mark": mr.MARK_REC, "seq": qr.SEQ_REC}
DTYPES = {"track": FLOW_TRACK_REC, **SIDE}
TOP_BYTES, TOP_PACKETS, TOP_DURATION, TOP_TCP_SYN, TOP_TCP_RST = range(5)
TOTALS = ("selected_packets", "keyed_packets", "none_packets", "overflow_packets", "selected_bytes", "keyed_bytes", "none_bytes",
          "overflow_bytes")


def auto_slots(flow_cap: int, factor: int = 2) -> int:
    s = 128
    while s < factor * flow_cap:
        s *= 2
    return s


class Life:
    """One life of a key: its packets since it was admitted, and the one-record side tables they add up to."""

    def __init__(self, key, number):
        self.key, self.number = key, number          # number: which life of this key (0 = the first)
        self.pk = []                                  # (batch, index in batch, frame, stamp, direction, hit)
        self.side = {t: np.zeros(1, d) for t, d in SIDE.items()}

    def track(self) -> np.ndarray:
        """The 104-byte record, by direct sums over the packets."""
        out = np.zeros(1, FLOW_TRACK_REC)
        r = out[0]
        klass, kb = self.key
        r["key"][:len(kb)] = np.frombuffer(kb, np.uint8)
        r["klass"] = klass
        first, last = self.pk[0], self.pk[-1]
        r["first_batch"], r["first"], r["first_ts"] = first[0] & 0xFFFFFFFF, first[1], first[3]
        r["last_batch"], r["last"], r["last_ts"] = last[0] & 0xFFFFFFFF, last[1], last[3]
        for d in (0, 1):
            r["packets"][d] = sum(1 for p in self.pk if p[4] == d)
            r["bytes"][d] = sum(min(len(p[2]), 65535) for p in self.pk if p[4] == d)
        return out

    def last_ts(self) -> int:
        return self.pk[-1][3]

    def tcp_state(self, flags: int) -> int:
        f = self.side["tcp"]["flags"][0]
        return tr.state(int(f[0]), int(f[1]), flags)


class SessionModel:
    def __init__(self, flags: int, flow_cap: int, slots: int = 0):
        self.flags, self.flow_cap, self.slots = flags, flow_cap, slots or auto_slots(flow_cap)
        self.lives = {}            # live keys in admission order -> Life
        self.seq = 0               # accepted update calls
        self.totals = dict.fromkeys(TOTALS, 0)
        self.batches, self.expires = [], []
        self.lives_of = {}         # key -> lives begun so far
        self.overflowed = set()    # keys that have overflowed and were not admitted since
        self.stats = {"returned": 0, "truncated": 0, "admitted_after_overflow": 0, "most_in_a_batch": 0, "spans_a_chunk": 0,
                      "expired_nothing": 0, "expired_all": 0}
        self._facts = {}

    # ---- what one frame is, by the pure-Python walks (cached per distinct frame)
    def facts(self, frame: bytes):
        got = self._facts.get(frame)
        if got is None:
            inputs, nbytes, klass = fr.key_of_frames([frame], bool(self.flags & ftr.L3_ONLY))
            k = int(klass[0])
            kb = bytes(inputs[0, :nbytes[0]])
            d = int(tr.directions(inputs, nbytes, klass, self.flags)[0])
            stored = ftr.canonical(kb, k)[0] if self.flags & ftr.BIDIRECTIONAL else kb
            got = self._facts[frame] = ((k, stored), d, tr.tcp_of_frame(frame), sr.facts_of_frame(frame))
        return got

    # ---- answers
    def live(self) -> list:
        """The live keys in admission order: the device's flow number of a key is its position."""
        return list(self.lives)

    def record(self, key, table: str) -> np.ndarray:
        """One record (a [1] array of the table's dtype): what that key's record must hold now."""
        life = self.lives[key]
        return life.track() if table == "track" else life.side[table].copy()

    def gone(self, call: int) -> list:
        return self.expires[call]["keys"]

    def packet(self, b: int, i: int) -> dict:
        e = self.batches[b]
        return {"flow_id": int(e["flow_id"][i]), "key": e["keys"][i], "seq": int(e["seq"][i]), "byte_off": int(e["byte_off"][i]),
                "keep": bool(fr.select_bits(e["seq_words"], e["n"])[i]), "session": bool(fr.select_bits(e["msel_words"], e["n"])[i])}

    def header(self) -> dict:
        return {"magic": MAGIC, "flags": self.flags, "flow_cap": self.flow_cap, "slots": self.slots, "n_flows": len(self.lives),
                "seq": self.seq & 0xFFFFFFFF, **self.totals, "reserved": [0] * 5}

    def table(self, name: str) -> np.ndarray:
        """The whole table: the live keys' records at their positions, zeros behind them."""
        out = np.zeros(self.flow_cap, DTYPES[name])
        for f, key in enumerate(self.lives):
            out[f] = self.record(key, name)[0]
        return out

    # ---- one batch through the chain: track, tcp / stat / mark, seq, mark select
    def update(self, frames, ts, select, hit, mark, max_packets=0, max_bytes=0, seq_flags=0, sel_op=mr.SET, sel_mask=1, sel_flags=0):
        """select, hit: bool arrays (select None = every packet). Returns what every call of the chain must give."""
        n = len(frames)
        sel = np.ones(n, bool) if select is None else np.asarray(select, bool)
        hit = np.asarray(hit, bool)
        info = [self.facts(bytes(f)) for f in frames]
        lens = np.array([min(len(f), 65535) for f in frames], np.int64)
        flow_id = np.full(n, ftr.UNSELECTED, np.uint32)
        groups = {}
        none_packets = none_bytes = keyed_bytes = 0
        for i in np.nonzero(sel)[0].tolist():
            key = info[i][0]
            if key[0] == fr.NONE:
                flow_id[i] = ftr.NONE_ID
                none_packets += 1
                none_bytes += int(lens[i])
            else:
                keyed_bytes += int(lens[i])
                groups.setdefault(key, []).append(i)
        # admission: a new key gets in, in batch order, while there is room; otherwise its packets overflow and it is not remembered
        new = over_flows = over_packets = over_bytes = 0
        admitted = {}
        for key, idx in groups.items():
            if key not in self.lives:
                if len(self.lives) < self.flow_cap:
                    number = self.lives_of.get(key, 0)
                    self.lives_of[key] = number + 1
                    self.lives[key] = Life(key, number)
                    new += 1
                    self.stats["returned"] += number > 0
                    if key in self.overflowed:
                        self.overflowed.discard(key)
                        self.stats["admitted_after_overflow"] += 1
                else:
                    self.overflowed.add(key)
                    over_flows += 1
                    over_packets += len(idx)
                    over_bytes += int(lens[idx].sum())
                    flow_id[idx] = ftr.OVERFLOW
                    continue
            admitted[key] = idx
        position = {key: f for f, key in enumerate(self.lives)}
        seq, off = np.full(n, qr.SEQ_NONE, np.uint32), np.full(n, qr.OFF_NONE, np.uint64)
        keep, marked = np.zeros(n, bool), np.zeros(n, bool)
        tcp_res = dict.fromkeys(("tcp_packets", "syn_packets", "fin_packets", "rst_packets"), 0)
        stat_res = dict.fromkeys(("ip_packets", "l4_packets", "tcp_packets"), 0)
        mark_res = dict.fromkeys(("marked_packets", "new_marked_flows"), 0)
        seq_res = dict.fromkeys(("numbered", "kept", "flows", "new_flows", "numbered_bytes", "kept_bytes"), 0)
        for key, idx in admitted.items():
            life, m = self.lives[key], len(idx)
            flow_id[idx] = position[key]
            zeros = np.zeros(m, np.uint32)
            dirs = np.array([info[i][1] for i in idx], np.int64)
            stamps = np.asarray(ts, np.uint64)[idx]
            r = tr.update(life.side["tcp"], zeros, [info[i][2][0] for i in idx], [info[i][2][1] for i in idx], dirs)
            for k in tcp_res:
                tcp_res[k] += r[k]
            r = sr.update(life.side["stat"], zeros, np.array([info[i][3] for i in idx], sr.FACTS), dirs, stamps)
            for k in stat_res:
                stat_res[k] += r[k]
            r = mr.update(life.side["mark"], zeros, lens[idx], fr.pack_bits(hit[idx]), mark, stamps)
            for k in mark_res:
                mark_res[k] += r[k]
            s, o, words, r = qr.number(life.side["seq"], zeros, lens[idx], None, max_packets, max_bytes, 0)
            seq[idx], off[idx], keep[idx] = s, o, fr.select_bits(words, m)
            for k in seq_res:
                seq_res[k] += r[k]
            life.pk += [(self.seq, i, bytes(frames[i]), int(ts[i]), info[i][1], bool(hit[i])) for i in idx]
            self.stats["most_in_a_batch"] = max(self.stats["most_in_a_batch"], m)
        # mark select sees the marks after this batch's update
        for key, idx in admitted.items():
            got = int(self.lives[key].side["mark"]["marks"][0]) & sel_mask
            marked[idx] = (got == sel_mask) if sel_flags & mr.ALL_BITS else (got != 0)
        numbered = flow_id < self.flow_cap
        unkeyed = sel & ~numbered
        if seq_flags & qr.KEEP_UNKEYED:
            keep |= unkeyed
        out = marked if sel_op == mr.SET else (keep & marked) if sel_op == mr.AND else (keep | marked) if sel_op == mr.OR else (keep & ~marked)
        # the sorted list of the numbering call: does a flow lie across a 16384-packet chunk boundary of it
        order = np.sort(flow_id[numbered])
        cuts = np.arange(16384, len(order), 16384)
        self.stats["spans_a_chunk"] += int((order[cuts - 1] == order[cuts]).sum())
        track_res = {"n": n, "n_selected": int(sel.sum()), "none_packets": none_packets, "batch_flows": len(groups), "new_flows": new,
                     "overflow_flows": over_flows, "overflow_packets": over_packets, "n_flows": len(self.lives), "seq": self.seq & 0xFFFFFFFF,
                     "status": 0, "keyed_bytes": keyed_bytes, "none_bytes": none_bytes, "overflow_bytes": over_bytes}
        t = self.totals
        t["selected_packets"] += int(sel.sum())
        t["keyed_packets"] += int(sel.sum()) - none_packets
        t["none_packets"] += none_packets
        t["overflow_packets"] += over_packets
        t["selected_bytes"] += keyed_bytes + none_bytes
        t["keyed_bytes"] += keyed_bytes
        t["none_bytes"] += none_bytes
        t["overflow_bytes"] += over_bytes
        self.seq += 1
        hits = int(hit.sum())
        e = {"n": n, "keys": [x[0] for x in info], "flow_id": flow_id, "track": track_res,
             "tcp": {"n": n, **tcp_res, "bad_ids": 0, "reserved": [0, 0]},
             "stat": {"n": n, **stat_res, "bad_ids": 0, "reserved": [0, 0, 0]},
             "mark": {"n": n, "hit_packets": hits, "marked_packets": mark_res["marked_packets"],
                      "unkeyed_hits": hits - mark_res["marked_packets"], "bad_ids": 0, "new_marked_flows": mark_res["new_marked_flows"],
                      "reserved": [0, 0]},
             "seq": seq, "byte_off": off, "seq_words": fr.pack_bits(keep),
             "seq_res": {"n": n, "selected": int(sel.sum()), "numbered": seq_res["numbered"], "unkeyed": int(unkeyed.sum()), "bad_ids": 0,
                         "kept": int(keep.sum()), "flows": seq_res["flows"], "new_flows": seq_res["new_flows"],
                         "numbered_bytes": seq_res["numbered_bytes"], "kept_bytes": seq_res["kept_bytes"], "reserved": [0, 0]},
             "msel_words": fr.pack_bits(out),
             "msel": {"n": n, "n_marked": int(marked.sum()), "n_out": int(out.sum()), "bad_ids": 0, "reserved": [0, 0, 0, 0]}}
        self.batches.append(e)
        return e

    # ---- an expire: plain (closed_idle None) or TCP-aware
    def expire(self, now: int, idle: int, closed_idle=None, expired_cap=None):
        """expired_cap None: the call's expired == NULL, every idle flow is dropped."""
        def older(life, limit):
            return life.last_ts() <= now and now - life.last_ts() > limit

        before = list(self.lives.items())
        leaving = [key for key, life in before
                   if older(life, idle) or (closed_idle is not None and life.tcp_state(self.flags) in (tr.CLOSED, tr.RESET)
                                            and older(life, closed_idle))]
        gone = leaving if expired_cap is None else leaving[:expired_cap]   # in admission order, cut at expired_cap
        gone_set = set(gone)
        e = {"keys": gone, "lives": [self.lives[k].number for k in gone],
             "track": np.concatenate([self.record(k, "track") for k in gone] + [np.zeros(0, FLOW_TRACK_REC)])}
        for t, d in SIDE.items():
            e[t] = np.concatenate([self.record(k, t) for k in gone] + [np.zeros(0, d)])
        remap, at = np.zeros(len(before), np.uint32), 0
        for f, (key, _) in enumerate(before):
            if key in gone_set:
                remap[f] = EXPIRED
                del self.lives[key]
            else:
                remap[f], at = at, at + 1
        e["remap"] = remap
        e["result"] = {"n_flows_before": len(before), "n_flows": len(self.lives), "n_idle": len(leaving), "n_expired": len(gone),
                       "status": 0, "reserved": [0, 0, 0]}
        self.stats["truncated"] += len(gone) < len(leaving)
        self.stats["expired_nothing"] += len(gone) == 0 and len(before) > 0
        self.stats["expired_all"] += len(gone) == len(before) > 0
        self.expires.append(e)
        return e

    # ---- the read-only views, from the live keys' records
    def top(self, metric: int, k: int, recs=None, tcps=None):
        keys = self.live()
        recs = self.table("track")[:len(keys)] if recs is None else recs[:len(keys)]
        tcps = self.table("tcp")[:len(keys)] if tcps is None else tcps[:len(keys)]
        if metric in (TOP_BYTES, TOP_PACKETS):
            name = "bytes" if metric == TOP_BYTES else "packets"
            vals = [(int(r[name][0]) + int(r[name][1])) & U64 for r in recs]
        elif metric == TOP_DURATION:
            vals = [int(r["last_ts"]) - int(r["first_ts"]) if r["last_ts"] >= r["first_ts"] else 0 for r in recs]
        else:
            vals = [int(t["syn_packets" if metric == TOP_TCP_SYN else "rst_packets"]) for t in tcps]
        order = sorted(range(len(keys)), key=lambda f: (-vals[f], f))[:k]
        thr = vals[order[-1]] if order else 0
        res = {"n_flows": len(keys), "n_top": len(order), "status": 0, "metric": metric,
               "n_ties": sum(1 for v in vals if v == thr) if order else 0, "reserved": 0, "threshold": thr,
               "total": sum(vals) & U64, "top_total": sum(vals[f] for f in order) & U64}
        return {"keys": [keys[f] for f in order], "ids": np.array(order, np.uint32), "values": np.array([vals[f] for f in order], np.uint64),
                "recs": recs[order] if order else recs[:0], "tcps": tcps[order] if order else tcps[:0], "result": res}

    def hosts(self, host_cap: int, slots: int = 0, recs=None, tcps=None):
        keys = self.live()
        recs = self.table("track")[:len(keys)] if recs is None else recs[:len(keys)]
        tcps = self.table("tcp")[:len(keys)] if tcps is None else tcps[:len(keys)]
        hosts, ends = {}, np.zeros(2 * len(keys), np.uint32)
        for f, (klass, kb) in enumerate(keys):
            alen, family = (4, 4) if klass in (fr.V4, fr.V4_L4) else (16, 6)
            r, t = recs[f], tcps[f]
            state = tr.state(int(t["flags"][0]), int(t["flags"][1]), self.flags)
            for role in (0, 1):
                hk = (family, kb[role * alen:(role + 1) * alen])
                h = hosts.get(hk)
                if h is None:
                    h = hosts[hk] = {"n": len(hosts), "first_flow": f, "flows": [0, 0], "packets": [0, 0], "bytes": [0, 0],
                                     "first_ts": U64, "last_ts": 0, "tcp_state": [0] * 7, "syn_flows": [0, 0], "syn": 0, "fin": 0, "rst": 0}
                ends[2 * f + role] = h["n"]
                h["flows"][role] += 1
                for name in ("packets", "bytes"):
                    h[name][0] += int(r[name][role])
                    h[name][1] += int(r[name][1 - role])
                h["first_ts"], h["last_ts"] = min(h["first_ts"], int(r["first_ts"])), max(h["last_ts"], int(r["last_ts"]))
                h["tcp_state"][state] += 1
                h["syn_flows"][0] += bool(int(t["flags"][role]) & tr.SYN)
                h["syn_flows"][1] += bool(int(t["flags"][1 - role]) & tr.SYN)
                for name, field in (("syn", "syn_packets"), ("fin", "fin_packets"), ("rst", "rst_packets")):
                    h[name] = (h[name] + int(t[field])) & 0xFFFFFFFF
        out = np.zeros(min(len(hosts), host_cap), FlowHostRec)
        for (family, addr), h in hosts.items():
            if h["n"] >= len(out):
                continue
            o = out[h["n"]]
            o["addr"][:len(addr)] = np.frombuffer(addr, np.uint8)
            o["family"], o["first_flow"], o["flows"] = family, h["first_flow"], h["flows"]
            o["packets"], o["bytes"] = [v & U64 for v in h["packets"]], [v & U64 for v in h["bytes"]]
            o["first_ts"], o["last_ts"], o["tcp_state"], o["syn_flows"] = h["first_ts"], h["last_ts"], h["tcp_state"], h["syn_flows"]
            o["syn_packets"], o["fin_packets"], o["rst_packets"] = h["syn"], h["fin"], h["rst"]
        res = {"n_flows": len(keys), "n_hosts": len(hosts), "n_written": len(out), "status": 0, "overflow_endpoints": 0,
               "slots": slots or auto_slots(self.flow_cap, 4), "hosts_v4": sum(1 for fam, _ in hosts if fam == 4),
               "hosts_v6": sum(1 for fam, _ in hosts if fam == 6),
               "packets_total": sum(int(r["packets"][0]) + int(r["packets"][1]) for r in recs) & U64,
               "bytes_total": sum(int(r["bytes"][0]) + int(r["bytes"][1]) for r in recs) & U64, "reserved": [0, 0]}
        return {"hosts": out, "endpoint_host": ends, "result": res}

    def checkpoint(self, k: int, host_cap: int):
        """Everything a checkpoint compares: the keys, the header, the five whole tables, every top-K and the hosts."""
        tables = {t: self.table(t) for t in TABLES}
        recs, tcps = tables["track"], tables["tcp"]
        return {"keys": self.live(), "lives": [life.number for life in self.lives.values()], "hdr": self.header(), **tables,
                "top": {m: self.top(m, k, recs, tcps) for m in range(5)}, "hosts": self.hosts(host_cap, 0, recs, tcps)}
