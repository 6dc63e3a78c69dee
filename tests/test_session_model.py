"""CPU: the whole flow chain in its host forms (bt_flow_track_update_host, the TCP / statistics / mark
updates, bt_flow_seq_host, bt_flow_mark_select_host, both expires, bt_flow_track_side_move_host for
every side table the expire did not carry, top-K and hosts at checkpoints) driven over the scenarios
of session_cases.py and held to session_ref.SessionModel, a model keyed by the flow key that never sees
a flow number. Every comparison is exact: bytes or integers."""
import numpy as np
import pytest

import flowtab_ref as ftr
import session_cases as sc
import session_ref as sm
from beatrice_amd import abi

SIDE_DTYPES = {"tcp": abi.FlowTcpRec, "stat": abi.FlowStatRec, "mark": abi.FlowMarkRec, "seq": abi.FlowSeqRec}


def run_host(name):
    """The scenario through the *_host calls: one observation per operation, in the shape session_cases.compare takes."""
    scn = sc.scenario(name)
    cap, flags = scn.flow_cap, scn.flags
    host = abi.HostFlowTracker(cap, flags, scn.slots)
    side = {t: np.zeros(cap, d) for t, d in SIDE_DTYPES.items()}
    host.tcp = side["tcp"]
    rng = np.random.default_rng(5)
    out = []
    for o in scn.ops:
        if o["op"] == "batch":
            n = len(o["frames"])
            nw = (n + 63) // 64
            data, desc = sc.pack(o["frames"])
            sel = None if o["select"] is None else sc.words(o["select"], rng)
            hit = sc.words(o["hit"], rng)
            ts = o["ts"] if n else None
            fid, track = host.update(data, desc, sel, ts)
            got = {"flow_id": fid.copy(), "track": track,
                   "tcp": abi.flow_tcp_update_host(data, desc, fid, flags, side["tcp"]),
                   "stat": abi.flow_stat_update_host(data, desc, fid, flags, side["stat"], ts=ts),
                   "mark": abi.flow_mark_update_host(desc, fid, hit, o["mark"], side["mark"], ts=ts),
                   "seq": np.full(n, 0x5A5A5A5A, np.uint32), "byte_off": np.full(n, 0x5A5A5A5A5A5A5A5A, np.uint64),
                   "seq_words": np.full(nw, 0x5A5A5A5A5A5A5A5A, np.uint64)}
            got["seq_res"] = abi.flow_seq_host(desc, fid, sel, side["seq"], o["mp"], o["mb"], o["seq_flags"], seq=got["seq"],
                                               byte_off=got["byte_off"], out_select=got["seq_words"])
            got["msel_words"], got["msel"] = abi.flow_mark_select_host(fid, side["mark"], o["sel_mask"], o["sel_op"], o["sel_flags"],
                                                                       base=got["seq_words"])
        elif o["op"] == "expire":
            c = o["cap"]
            if o["closed_idle"] is None:
                exp, remap, res = host.expire(o["now"], o["idle"], c)
                moved = ("tcp", "stat", "mark", "seq")
                got = {}
            else:   # the TCP table goes with the expire itself
                exp, exp_tcp, remap, res = host.expire_tcp(o["now"], o["idle"], o["closed_idle"], c)
                moved = ("stat", "mark", "seq")
                got = {"tcp": exp_tcp}
            got.update({"track": exp, "remap": remap[:res["n_flows_before"]].copy(), "result": res})
            for t in moved:   # each with its own expired_side
                got[t] = abi.flow_track_side_move_host(side[t], remap, res, c)
        else:
            hdr = host.header()
            lay = host.layout
            got = {"hdr": hdr, "track": host.state[lay["records"]:lay["records"] + 104 * cap].copy().view(sm.FLOW_TRACK_REC),
                   **{t: side[t].copy() for t in side}, "top": {}}
            for m in range(5):
                ids, vals, recs, tcps, res = abi.flow_track_top_host(host.state, m, scn.k, side["tcp"])
                got["top"][m] = {"ids": ids, "values": vals, "recs": recs, "tcps": tcps, "result": res}
            hosts, ends, res = abi.flow_track_hosts_host(host.state, scn.host_cap, 0, side["tcp"])
            got["hosts"] = {"hosts": hosts, "endpoint_host": ends, "result": res}
        out.append(got)
    return out


@pytest.mark.parametrize("name", sc.SCENARIOS)
def test_the_host_chain_is_what_each_key_s_packets_add_up_to(name):
    sc.assert_not_vacuous(name)   # on the model alone, before anything is compared
    sc.compare(name, run_host(name), "host: ")


def test_the_model_answers_by_key():
    """live(), record(), gone() and packet() on the smallest scenario: a key's flow number is its position,
    a key that left and came back is a new life whose numbering starts at zero."""
    model, exp = sc.expected("l3_64")
    scn = sc.scenario("l3_64")
    assert model.live() == exp[-1]["keys"] and len(model.expires) == 3 and model.gone(2) and not model.live() == model.gone(2)
    last = max(j for j, o in enumerate(scn.ops) if o["op"] == "batch")
    b = sum(1 for o in scn.ops[:last + 1] if o["op"] == "batch") - 1
    e = model.batches[b]
    seen = set()
    for i in range(e["n"]):
        p = model.packet(b, i)
        if p["flow_id"] < scn.flow_cap:
            assert model.live()[p["flow_id"]] == p["key"]
            if p["key"] not in seen:   # everything was dropped by the expire before this batch
                assert p["seq"] == 0 and p["byte_off"] == 0
                seen.add(p["key"])
    assert seen and all(int(model.record(k, "seq")["packets"][0]) == int(model.record(k, "track")["packets"].sum()) for k in seen)
    assert scn.flags & ftr.BIDIRECTIONAL
