"""The flow tracker's expected values, restated in Python and independent of the code under test: a
dict over (class, key bytes) that lives across batches. Each batch's flows come from
flowtab_ref.expected (keys from flow_ref), then the merge, the overflow rule and the expiry are
restated here. Every output of bt_flow_track_update_* / _expire_* comes out of Tracker: flow_id,
the result, the header and the records as the 104-byte dtype."""
import numpy as np

import flowtab_ref as ftr

EXPIRED = 0xFFFFFFFB
MAGIC = 0x4B525446

FLOW_TRACK_REC = np.dtype({
    "names": ["key", "klass", "pad", "first_batch", "last_batch", "first", "last", "packets", "bytes", "first_ts", "last_ts"],
    "formats": [("u1", 36), "u1", ("u1", 3), "<u4", "<u4", "<u4", "<u4", ("<u8", 2), ("<u8", 2), "<u8", "<u8"],
    "offsets": [0, 36, 37, 40, 44, 48, 52, 56, 72, 88, 96],
    "itemsize": 104,
})
TOTALS = ("selected_packets", "keyed_packets", "none_packets", "overflow_packets", "selected_bytes", "keyed_bytes", "none_bytes",
          "overflow_bytes")


def auto_slots(flow_cap: int) -> int:
    s = 128
    while s < 2 * flow_cap:
        s *= 2
    return s


class Tracker:
    def __init__(self, flow_cap: int, flags: int = 0, slots: int = 0):
        self.flow_cap, self.flags, self.slots = flow_cap, flags, slots or auto_slots(flow_cap)
        self.flows = []    # record f = flow number f: dicts
        self.table = {}    # (class, key bytes) -> flow number
        self.seq = 0
        self.totals = dict.fromkeys(TOTALS, 0)

    def update(self, inputs, nbytes, klass, lens, select=None, ts=None, batch_ts=0) -> dict:
        """One batch of n packets with these keys (flow_ref's triple) and frame lengths."""
        n = len(klass)
        batch = ftr.expected(inputs, nbytes, klass, lens, self.flags, select)
        stamp = (lambda i: int(ts[i])) if ts is not None else (lambda i: int(batch_ts))
        mapped = []
        new = over_flows = over_packets = over_bytes = 0
        for f in batch["flows"]:
            k = (int(f["klass"]), f["key"].tobytes())
            p, b = [int(x) for x in f["packets"]], [int(x) for x in f["bytes"]]
            at = self.table.get(k)
            if at is not None:
                r = self.flows[at]
                r["packets"] = [r["packets"][0] + p[0], r["packets"][1] + p[1]]
                r["bytes"] = [r["bytes"][0] + b[0], r["bytes"][1] + b[1]]
                r["last_batch"], r["last"], r["last_ts"] = self.seq, int(f["last"]), stamp(int(f["last"]))
            elif len(self.flows) < self.flow_cap:
                at = self.table[k] = len(self.flows)
                self.flows.append({"klass": k[0], "key": k[1], "first_batch": self.seq, "last_batch": self.seq,
                                   "first": int(f["first"]), "last": int(f["last"]), "packets": p, "bytes": b,
                                   "first_ts": stamp(int(f["first"])), "last_ts": stamp(int(f["last"]))})
                new += 1
            else:
                at = ftr.OVERFLOW
                over_flows += 1
                over_packets += sum(p)
                over_bytes += sum(b)
            mapped.append(at)
        local = batch["flow_id"]
        lut = np.array(mapped + [0], np.uint32)
        flow_id = np.where(local < 0xFFFFFFFC, lut[np.minimum(local, len(mapped))], local).astype(np.uint32)
        br = batch["result"]
        res = {"n": n, "n_selected": br["n_selected"], "none_packets": br["none_packets"], "batch_flows": br["n_flows"],
               "new_flows": new, "overflow_flows": over_flows, "overflow_packets": over_packets, "n_flows": len(self.flows),
               "seq": self.seq, "status": 0, "keyed_bytes": br["keyed_bytes"], "none_bytes": br["none_bytes"],
               "overflow_bytes": over_bytes}
        self.seq += 1
        t = self.totals
        t["selected_packets"] += res["n_selected"]
        t["keyed_packets"] += res["n_selected"] - res["none_packets"]
        t["none_packets"] += res["none_packets"]
        t["overflow_packets"] += over_packets
        t["selected_bytes"] += res["keyed_bytes"] + res["none_bytes"]
        t["keyed_bytes"] += res["keyed_bytes"]
        t["none_bytes"] += res["none_bytes"]
        t["overflow_bytes"] += over_bytes
        return {"flow_id": flow_id, "result": res}

    def expire(self, now: int, idle: int, expired_cap=None) -> dict:
        """expired_cap None: the call's expired == NULL, every idle flow is dropped."""
        before = len(self.flows)
        idle_flows = [f for f, r in enumerate(self.flows) if r["last_ts"] <= now and now - r["last_ts"] > idle]
        gone = idle_flows if expired_cap is None else idle_flows[:expired_cap]
        gone_set = set(gone)
        remap = np.zeros(before, np.uint32)
        live = []
        for f, r in enumerate(self.flows):
            if f in gone_set:
                remap[f] = EXPIRED
            else:
                remap[f] = len(live)
                live.append(r)
        expired = self._pack([self.flows[f] for f in gone])
        self.flows = live
        self.table = {(r["klass"], r["key"]): f for f, r in enumerate(live)}
        return {"expired": expired, "remap": remap,
                "result": {"n_flows_before": before, "n_flows": len(live), "n_idle": len(idle_flows), "n_expired": len(gone),
                           "status": 0, "reserved": [0, 0, 0]}}

    @staticmethod
    def _pack(flows) -> np.ndarray:
        out = np.zeros(len(flows), FLOW_TRACK_REC)
        for f, r in enumerate(flows):
            out[f]["key"][:len(r["key"])] = np.frombuffer(r["key"], np.uint8)
            for name in ("klass", "first_batch", "last_batch", "first", "last", "packets", "bytes", "first_ts", "last_ts"):
                out[f][name] = r[name]
        return out

    def records(self, whole: bool = False) -> np.ndarray:
        """The live records; whole: all flow_cap of them, zeros behind the live ones."""
        out = self._pack(self.flows)
        return np.concatenate([out, np.zeros(self.flow_cap - len(out), FLOW_TRACK_REC)]) if whole else out

    def header(self) -> dict:
        return {"magic": MAGIC, "flags": self.flags, "flow_cap": self.flow_cap, "slots": self.slots, "n_flows": len(self.flows),
                "seq": self.seq, **self.totals, "reserved": [0] * 5}
