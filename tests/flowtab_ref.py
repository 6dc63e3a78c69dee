"""The flow table's expected values, restated in Python and independent of the code under test: a
dict over (class, key bytes), the keys from flow_ref.key_of_rec on the goldens' reference-made
records or from flow_ref.walk for crafted frames. Every output of bt_flow_table_device /
bt_flow_table_host comes out of expected(): flow_id, flows as the 80-byte dtype, result."""
import numpy as np

import flow_ref as fr

UNSELECTED, NONE_ID, OVERFLOW = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD
L3_ONLY, BIDIRECTIONAL = 1, 2

FLOW_REC = np.dtype({
    "names": ["key", "klass", "pad", "first", "last", "packets", "bytes", "reserved"],
    "formats": [("u1", 36), "u1", ("u1", 3), "<u4", "<u4", ("<u4", 2), ("<u8", 2), "<u8"],
    "offsets": [0, 36, 37, 40, 44, 48, 56, 72],
    "itemsize": 80,
})


def auto_slots(n: int) -> int:
    s = 128
    while s < 2 * n:
        s *= 2
    return s


def canonical(key: bytes, klass: int):
    """(stored key, direction): endpoint A = source address + source port, B = the destination's,
    compared as byte strings; A > B swaps them and counts in direction 1."""
    if klass == fr.NONE:
        return key, 0
    alen = 4 if klass in (fr.V4, fr.V4_L4) else 16
    ports = key[2 * alen:]
    a, b = key[:alen] + ports[0:2], key[alen:2 * alen] + ports[2:4]
    if a <= b:
        return key, 0
    return key[alen:2 * alen] + key[:alen] + ports[2:4] + ports[0:2], 1


def distinct_keys(inputs, nbytes, klass, bidirectional=False):
    """Per distinct row of (class, key): (stored key bytes, direction); and every packet's row number."""
    rows = np.concatenate([np.asarray(klass, np.uint8)[:, None], np.asarray(inputs, np.uint8)], axis=1)
    uniq, inverse = np.unique(rows, axis=0, return_inverse=True)
    out = []
    for u in uniq:
        k = int(u[0])
        kb = bytes(u[1:1 + {fr.NONE: 0, fr.V4: 8, fr.V4_L4: 12, fr.V6: 32, fr.V6_L4: 36}[k]])
        out.append(canonical(kb, k) if bidirectional else (kb, 0))
    return out, inverse.reshape(-1)


def expected(inputs, nbytes, klass, lens, flags=0, select=None, flow_cap=None, slots=0) -> dict:
    """Every output for n packets with these keys (flow_ref.key_of_rec's triple), classes and frame
    lengths. flow_cap None: every flow is written."""
    n = len(klass)
    sel = fr.select_bits(select, n)
    lens = np.minimum(np.asarray(lens, np.int64), 65535)
    stored, row = distinct_keys(inputs, nbytes, klass, bool(flags & BIDIRECTIONAL)) if n else ([], np.zeros(0, np.int64))
    table, flows = {}, []
    flow_id = np.full(n, UNSELECTED, np.uint32)
    none_packets = none_bytes = keyed_bytes = 0
    for i in np.nonzero(sel)[0].tolist():
        k = int(klass[i])
        if k == fr.NONE:
            flow_id[i] = NONE_ID
            none_packets += 1
            none_bytes += int(lens[i])
            continue
        keyed_bytes += int(lens[i])
        kb, d = stored[row[i]]
        f = table.get((k, kb))
        if f is None:
            f = table[(k, kb)] = len(flows)
            flows.append({"key": kb, "klass": k, "first": i, "last": i, "packets": [0, 0], "bytes": [0, 0]})
        rec = flows[f]
        rec["last"] = i
        rec["packets"][d] += 1
        rec["bytes"][d] += int(lens[i])
        flow_id[i] = f
    cap = len(flows) if flow_cap is None else flow_cap
    out = np.zeros(min(cap, len(flows)), FLOW_REC)
    for f, rec in enumerate(flows[:len(out)]):
        out[f]["key"][:len(rec["key"])] = np.frombuffer(rec["key"], np.uint8)
        out[f]["klass"], out[f]["first"], out[f]["last"] = rec["klass"], rec["first"], rec["last"]
        out[f]["packets"], out[f]["bytes"] = rec["packets"], rec["bytes"]
    res = {"n": n, "n_selected": int(sel.sum()), "n_flows": len(flows), "n_written": len(out),
           "none_packets": none_packets, "overflow_packets": 0, "slots": slots or auto_slots(n), "reserved": 0,
           "klass_flows": [sum(1 for r in flows if r["klass"] == k) for k in range(5)], "pad": 0,
           "none_bytes": none_bytes, "keyed_bytes": keyed_bytes}
    return {"flow_id": flow_id, "flows": out, "result": res}


def of_frames(frames, flags=0, select=None, flow_cap=None, slots=0) -> dict:
    """expected() for crafted frames: the keys from flow_ref.walk."""
    inputs, nbytes, klass = fr.key_of_frames(frames, bool(flags & L3_ONLY))
    return expected(inputs, nbytes, klass, [len(f) for f in frames], flags, select, flow_cap, slots)
