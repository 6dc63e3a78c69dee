"""CPU: the host copies of the flow kernels' layer walk held to the restatements and to each other.
One batch (flow_walk_cases.py: seven seed frames at every length from 0 to their own, so every
"is it inside the frame" rule of the walk meets both its sides) goes through bt_flow_hash_host,
bt_flow_table_host and bt_flow_tcp_update_host under every flag combination. Each must equal
flow_ref / flowtab_ref / flowtcp_ref, and they must agree with one another on what the walk
decides: a packet's class, which packets are one flow, and which packets are TCP."""
import numpy as np
import pytest

import flow_ref as fr
import flow_walk_cases as wc
import flowtab_ref as ftr
import flowtcp_ref as tr
from beatrice_amd import abi


def ref_keys(l3_only):
    return fr.key_of_frames(wc.batch()[0], l3_only)


def test_the_sweep_meets_every_class_and_both_sides_of_every_rule():
    frames = wc.batch()[0]
    _, _, klass = ref_keys(False)
    assert set(klass.tolist()) == {fr.NONE, fr.V4, fr.V4_L4, fr.V6, fr.V6_L4}
    whole = {name: fr.walk(seed)[1] for name, seed in wc.SEEDS.items()}
    assert whole == {"v4_tcp_ihl6": fr.V4_L4, "tag_v4_udp": fr.V4_L4, "v6_udp": fr.V6_L4, "v4_fragment_mf": fr.V4,
                     "v4_proto1": fr.V4, "three_tags": fr.NONE, "qinq_v6_tcp": fr.V6_L4}
    tcp, _ = tr.tcp_of_frames(frames)
    # the whole TCP header of the IHL-6 seed ends at 14 + 24 + 20, that of the double-tagged IPv6 seed at 22 + 40 + 20
    assert int(tcp.sum()) == (100 - 58 + 1) + (86 - 82 + 1)


@pytest.mark.parametrize("l3_only", [False, True])
def test_host_fanout_equals_the_restatement(l3_only):
    h, klass, queue = wc.host_whole()["fanout"][l3_only]
    inputs, nbytes, want_klass = ref_keys(l3_only)
    assert (klass == want_klass).all()
    want_h = fr.toeplitz_many(fr.DEFAULT_KEY, inputs, nbytes)
    assert (h == want_h).all()
    assert (queue == fr.default_reta(wc.QUEUES)[want_h & 127]).all()


@pytest.mark.parametrize("flags", wc.ALL_FLAGS)
def test_host_table_and_tcp_update_equal_the_restatements(flags):
    frames = wc.batch()[0]
    flow_id, flows, res = wc.host_whole()["table"][flags]
    keys = ref_keys(bool(flags & ftr.L3_ONLY))
    want = ftr.expected(*keys, [len(f) for f in frames], flags, flow_cap=len(frames))
    assert (flow_id == want["flow_id"]).all() and res == want["result"]
    assert flows.tobytes() == want["flows"].tobytes()
    table, tres = wc.host_whole()["tcp"][flags]
    tcp, fl = tr.tcp_of_frames(frames)
    want_table = np.zeros(len(frames), tr.TCP_REC)
    want_res = tr.update(want_table, want["flow_id"], tcp, fl, tr.directions(*keys, flags))
    assert tres == want_res and table.tobytes() == want_table.tobytes()


@pytest.mark.parametrize("flags", wc.ALL_FLAGS)
def test_the_host_calls_agree_with_one_another(flags):
    frames = wc.batch()[0]
    l3_only = bool(flags & ftr.L3_ONLY)
    h, klass, _ = wc.host_whole()["fanout"][l3_only]
    flow_id, flows, res = wc.host_whole()["table"][flags]
    assert res["n_written"] == res["n_flows"] and res["overflow_packets"] == 0
    # a packet's class is the same in fan-out and table
    keyed = flow_id < res["n_flows"]
    assert ((flow_id == abi.FLOW_ID_NONE) == (klass == fr.NONE)).all() and (keyed == (klass != fr.NONE)).all()
    assert (flows["klass"][flow_id[keyed]] == klass[keyed]).all()
    # two packets with one unidirectional flow id have one RSS hash
    if not flags & ftr.BIDIRECTIONAL:
        first = flows["first"][flow_id[keyed]]
        assert (h[keyed] == h[first]).all()
        # six seeds have a key and addresses of their own; with ports, four of them are a second flow once cut short
        assert res["n_flows"] == (6 if l3_only else 10)
    # tcp_packets is the number of frames the reference walk calls TCP, whatever the table's flags
    tcp, _ = tr.tcp_of_frames(frames)
    assert wc.host_whole()["tcp"][flags][1]["tcp_packets"] == int(tcp.sum()) > 0
