"""GPU: the PAYLOAD forms BT_OPT_PAYLOAD_EXTENDED adds to the kernel — \\b \\B (byte DFAs whose
states carry the previous byte's word class), POSIX bracket classes and the wide DFA form
(16-bit state ids, eval_payload's wide walk) — decided on the device and compared with the
compiled reference's recorded outcomes (tests/golden/regex_ext.*, make_regex_ext.py): by
descriptors at every 16-B residue, at fixed strides of 64 and 128 bytes, inside a chain
between built-in filters, and through a group. A default context keeps them on the host."""
import ctypes
import json
import os

import numpy as np
import pytest

from beatrice_amd import abi, synth
from conftest import GOLDEN
from golden_util import compare_decisions

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    z = np.load(os.path.join(GOLDEN, "regex_ext.npz"), allow_pickle=False)
    with open(os.path.join(GOLDEN, "regex_ext.json")) as fh:
        meta = json.load(fh)
    return {k: z[k] for k in z.files}, meta


@pytest.fixture(scope="module")
def ext_ctx():
    ctx = abi.Context(0, flags=abi.OPT_PAYLOAD_EXTENDED)
    yield ctx
    ctx.close()


def _payload(expr):
    return [{"type": abi.PAYLOAD, "expr": expr, "priority": 1}]


def _decide(ctx, data, desc, n, stride=0):
    run = abi.DeviceRun(ctx, data, desc, n, stride=stride, records=False)
    run.run()
    dec = run.fetch()["decide"]
    run.free()
    return dec


def test_default_context_keeps_extended_patterns_on_host(gpu_ctx, fx):
    _, meta = fx
    for expr in ("\\bfoo", "[[:alpha:]]", meta["wide"][0]):
        assert expr in meta["patterns"]
        assert abi.KINDS[gpu_ctx.compile(_payload(expr))[0].kind] == "HOST", expr


def test_extended_patterns_decide_on_gpu(ext_ctx, fx):
    g, meta = fx
    n = len(g["desc"])
    for p, expr in enumerate(meta["patterns"]):
        f = _payload(expr)
        assert abi.KINDS[ext_ctx.compile(f)[0].kind] == "PAYLOAD", f"/{expr}/ stayed on the host"
        dec = _decide(ext_ctx, g["data"], g["desc"], n)
        assert not np.any((dec >> 6) == 3), f"/{expr}/: BT_DECIDE_HOST codes"
        compare_decisions(dec, g["code"][p], g["src"][p], f, where=f"regex_ext /{expr}/")


@pytest.mark.parametrize("stride", [64, 128])
def test_extended_patterns_fixed_stride(ext_ctx, fx, stride):
    """The frames that fit, zero-padded to the stride (so the window runs on into the padding):
    64-B frames take the 17-dword LDS rows."""
    g, meta = fx
    n = len(g["desc"])
    off, ln = synth.desc_off(g["desc"]), synth.desc_len(g["desc"])
    keep = np.nonzero(ln <= stride)[0]
    assert 2 * len(keep) >= n, f"only {len(keep)} of {n} frames fit a {stride}-B stride"
    buf = np.zeros(len(keep) * stride + 256, np.uint8)
    for j, i in enumerate(keep):
        o, m = int(off[i]), int(ln[i])
        buf[j * stride:j * stride + m] = g["data"][o:o + m]
    for p, expr in enumerate(meta["patterns"]):
        f = _payload(expr)
        assert abi.KINDS[ext_ctx.compile(f)[0].kind] == "PAYLOAD", f"/{expr}/ stayed on the host"
        dec = _decide(ext_ctx, buf[: len(keep) * stride], None, len(keep), stride=stride)
        want = g[f"code{stride}"][p][keep]
        assert want.max() <= 1
        assert not np.any((dec >> 6) == 3), f"/{expr}/ stride {stride}: BT_DECIDE_HOST codes"
        compare_decisions(dec, want, np.zeros(len(keep), np.uint8), f, where=f"regex_ext stride {stride} /{expr}/")


def test_extended_chain(ext_ctx, fx):
    g, meta = fx
    prog = ext_ctx.compile(meta["chain"])
    assert [abi.KINDS[s.kind] for s in prog] == ["PROTO_EQ", "PAYLOAD", "PAYLOAD", "PORT"]
    dec = _decide(ext_ctx, g["data"], g["desc"], len(g["desc"]))
    assert not np.any((dec >> 6) == 3)
    compare_decisions(dec, g["chain_code"], g["chain_src"], meta["chain"], where="regex_ext chain")
    assert 0 < int(((dec >> 6) == 0).sum()) < len(dec)


def test_extended_group(fx):
    """Two members sharing device 0 inherit the option through bt_opts and decide a \\b program
    as the single context and the reference do."""
    g, meta = fx
    expr = "\\bGET\\b|\\bPOST\\b"
    p, f = meta["patterns"].index(expr), _payload(expr)
    grp = abi.Group([0, 0], flags=abi.OPT_GROUP_SHARED_DEVICE | abi.OPT_PAYLOAD_EXTENDED, host_chunk_packets=512)
    try:
        grp.compile(f)
        slot = abi.FilterSlot()
        cnt = ctypes.c_uint32(0)
        abi._check(abi.lib().bt_filter_program(grp.member(1), ctypes.byref(slot), 1, ctypes.byref(cnt)))
        assert cnt.value == 1 and abi.KINDS[slot.kind] == "PAYLOAD"
        out = grp.run_host(g["data"], g["desc"], records=False)
    finally:
        grp.close()
    ctx = abi.Context(0, flags=abi.OPT_PAYLOAD_EXTENDED, host_chunk_packets=512)
    try:
        ctx.compile(f)
        one = ctx.run_host(g["data"], g["desc"], records=False)
    finally:
        ctx.close()
    assert np.array_equal(out["decide"], one["decide"])
    assert not np.any((out["decide"] >> 6) == 3)
    compare_decisions(out["decide"], g["code"][p], g["src"][p], f, where="regex_ext group")


def test_wide_slots_that_overflow_the_pool_stay_on_host(ext_ctx):
    """(ab)*c.{8}d is an 11.6 KB wide table and (ab)*c.{7}d a 6 KB one: the 16 KiB pool holds one
    of each size but not both, in either order."""
    big, small = "(ab)*c.{8}d", "(ab)*c.{7}d"
    for order in ([big, small, small], [small, big, small]):
        fs = [{"type": abi.PAYLOAD, "expr": e, "priority": -k} for k, e in enumerate(order)]
        kinds = [abi.KINDS[s.kind] for s in ext_ctx.compile(fs)]
        assert kinds[0] == "PAYLOAD" and kinds[1] == "HOST", kinds
        pool = ctypes.c_uint32(0)
        abi._check(abi.lib().bt_filter_dfa_pool(ext_ctx.h, None, 0, ctypes.byref(pool)))
        assert 0 < pool.value <= 16384
