"""Restatement of bt_flow_follow_* (include/beatrice_gpu.h, "per-flow TCP reassembly, exported") as a plain
loop over Python integers, written from the header's text: the rules 1. - 8. of the reassembly in their
order, as flowreasm_ref.Reasm states them, and on top of them the bytes, the runs and the places. Nothing
here calls the code under test."""
import numpy as np

import flowreasm_ref as rr
import flowstream_ref as sr

NEW, HOLE = 2, 4
NO_PLACE = (1 << 64) - 1
RUN = np.dtype({"names": ["flow", "flags", "at", "pos", "len"], "formats": ["<u4", "<u4", "<u8", "<i8", "<u8"],
                "offsets": [0, 4, 8, 16, 24], "itemsize": 32})
FRESULT = ("total", "written", "n_runs", "runs_written")


class Follow(rr.Reasm):
    """The reassembly records of a table of `cap` flows; blob None: the plain follow, no pattern."""

    def __init__(self, cap: int, blob, table_flags: int = 0, start=None):
        self.cap, self.flags = cap, table_flags
        self.masks = sr.Masks(blob) if blob is not None else None
        self.state = {}
        if start is not None:
            for f in range(cap):
                for d in range(2):
                    r = start[f]["d"][d]
                    if any(int(r[name]) for name in rr.DIR_REC.names):
                        self.state[(f, d)] = {name: int(r[name]) for name in rr.DIR_REC.names}

    def follow(self, frames, flow_id, off, select=None, cap=None, run_cap=None):
        """One call. Returns (hit words, rest words, result dict, every delivered byte, every run as a RUN
        array, place as n u64, the follow's result dict for the capacities cap and run_cap; None = enough)."""
        n = len(frames)
        nw = (n + 63) // 64
        hit, rest = np.zeros(nw, np.uint64), np.zeros(nw, np.uint64)
        r = {k: 0 for k in rr.RESULT}
        r["n"] = n
        hits_before = {k: st["hit_packets"] for k, st in self.state.items()}
        streams = {}
        for i in range(n):
            if select is not None and not (int(select[i >> 6]) >> (i & 63)) & 1:
                continue
            r["selected"] += 1
            if int(off[i]) == rr.OFF_NONE:
                rest[i >> 6] |= np.uint64(1 << (i & 63))
            f = int(flow_id[i])
            if f >= self.cap:
                r["unkeyed" if f in rr.SENTINELS else "bad_ids"] += 1
                continue
            if int(off[i]) == rr.OFF_NONE:
                continue
            pl = rr.tcp_payload(frames[i])
            if pl is None:
                continue
            start, end, syn = pl
            d = sr.direction(frames[i], self.flags)
            st = self.rec(f, d)
            ds = int(off[i]) + syn
            de = ds + (end - start)
            if st["have"]:
                nxt = st["next"]
                if de <= nxt:                       # 2.
                    st["late_packets"] += 1
                    st["late_bytes"] += end - start
                    r["late_packets"] += 1
                    continue
                base, trim = nxt, max(0, nxt - ds)   # 1., 3.
            else:
                base, trim = rr.NEW_BASE, 0
            rel = ds + trim - base                  # 4.
            if rel < 0 or rel > rr.REL_MAX:
                r["far_packets"] += 1
                continue
            st["dup_bytes"] += trim
            streams.setdefault((f, d), []).append((rel, i, bytes(frames[i][start + trim:end])))
        out, runs, place = bytearray(), [], np.full(n, NO_PLACE, np.uint64)
        hit_flows = set()
        for (f, d) in sorted(streams):              # ascending flow << 1 | direction
            segs = streams[(f, d)]
            st = self.rec(f, d)
            segs.sort(key=lambda s: (s[0], s[1]))   # 5.
            had = bool(st["have"])
            base = st["next"] if had else rr.NEW_BASE
            D = st["d"] if had and self.masks else 0
            hi = 0 if had else segs[0][0]
            first = True
            for rel, i, data in segs:               # 6.
                hole = rel > hi
                if hole:
                    st["holes"] += 1
                    st["hole_bytes"] += rel - hi
                    r["holes"] += 1
                    D = 0
                if rel + len(data) <= hi:
                    st["dup_packets"] += 1
                    st["dup_bytes"] += len(data)
                    r["dup_packets"] += 1
                    continue
                skip = max(hi - rel, 0)
                if first or hole:                   # a run starts: the stream's first delivering segment, or rel > hi
                    runs.append([f, d | (0 if had else NEW) | (HOLE if hole else 0), len(out), base + max(rel, hi), 0])
                first = False
                st["dup_bytes"] += skip
                place[i] = len(out)
                out += data[skip:]
                runs[-1][4] += len(data) - skip
                got = False
                if self.masks:
                    D, got = self.masks.run(D, data[skip:])
                st["stream_packets"] += 1
                r["stream_packets"] += 1
                r["stream_bytes"] += len(data) - skip
                if got:
                    st["hit_packets"] += 1
                    r["hit_packets"] += 1
                    hit[i >> 6] |= np.uint64(1 << (i & 63))
                    hit_flows.add(f)
                hi = max(hi, rel + len(data))
            st["next"] = base + hi                  # 7.
            st["have"], st["d"] = 1, D
        r["new_hit_flows"] = sum(1 for f in hit_flows if not hits_before.get((f, 0), 0) and not hits_before.get((f, 1), 0))
        arr = np.zeros(len(runs), RUN)
        for k, row in enumerate(runs):
            arr[k] = tuple(row)
        total = len(out)
        fres = {"total": total, "written": total if cap is None else min(total, cap), "n_runs": len(runs),
                "runs_written": len(runs) if run_cap is None else min(len(runs), run_cap)}
        return hit, rest, r, bytes(out), arr, place, fres
