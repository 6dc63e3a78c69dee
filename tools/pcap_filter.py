"""Filter a classic pcap capture on the GPU: the records whose packets pass every filter are
written, verbatim and in order, behind the input's global header (bt_pcap_filter).

Usage: python tools/pcap_filter.py --in a.pcap --out b.pcap --filter TYPE:EXPR[:PRIO] ...
  TYPE  bpf | protocol | ip_range | port_range | payload   (PacketFilter::FilterType)
  EXPR  the filter's expression, e.g. udp, 10.0.0.0/8, 1000-2000, "GET|POST"
  PRIO  an integer; higher priorities are evaluated first (default 0). A trailing :INTEGER is
        always read as the priority.
Prints the result counts as one JSON line. A filter the GPU cannot decide (a PAYLOAD regex
outside its subset) is refused.
"""
from __future__ import annotations

import argparse
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from beatrice_amd import abi  # noqa: E402

TYPES = {"bpf": abi.BPF, "protocol": abi.PROTOCOL, "ip_range": abi.IP_RANGE, "port_range": abi.PORT_RANGE,
         "payload": abi.PAYLOAD}


def parse_filter(text: str) -> dict:
    name, sep, rest = text.partition(":")
    if not sep or name.lower() not in TYPES:
        raise SystemExit(f"--filter {text!r}: want TYPE:EXPR[:PRIO] with TYPE one of {', '.join(TYPES)}")
    prio = 0
    m = re.fullmatch(r"(.*):(-?\d+)", rest, flags=re.S)
    if m:
        rest, prio = m.group(1), int(m.group(2))
    return {"type": TYPES[name.lower()], "expr": rest, "priority": prio}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--in", dest="src", required=True)
    ap.add_argument("--out", dest="dst", required=True)
    ap.add_argument("--filter", action="append", default=[], metavar="TYPE:EXPR[:PRIO]")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    filters = [parse_filter(f) for f in a.filter]
    data = np.fromfile(a.src, np.uint8)
    ctx = abi.Context(a.device)
    try:
        ctx.compile(filters)
        out, res = ctx.pcap_filter(data)
    except abi.BtError as e:
        raise SystemExit(f"pcap_filter: {e}")
    finally:
        ctx.close()
    with open(a.dst, "wb") as fh:
        fh.write(out)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
