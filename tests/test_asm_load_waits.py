"""The batched loads of K3's two new kernels, read from the gfx950 assembly (tools/asm_load_waits.py; no GPU): k3_in_part<1> issues
every load of a trip — eight next-destination words and eight accumulator pairs — before the first wait that retires one of them, and
the eight destination loads ahead of the loop likewise; k3_node_features_lanes issues the slice loads of a node as whole batches (24
16-byte loads for 64 slices, 18 for the last 48).  hipcc decides this, not the source: a load under a condition of its own becomes a
block of its own and is waited for there, which is what form 0 of the scan compiles to (and this test shows on it).

Only loads and waits are looked at.  A RUN is a stretch of loads in program order that no wait cuts: `s_waitcnt vmcnt(n)` leaves the
n youngest loads in flight (loads return in order), so it retires a load of the current run exactly when n is smaller than the run's
length so far — whatever was in flight before the run.  Loads are told apart by width: in both kernels the 16-byte loads
(global_load_dwordx4) are the accumulator pairs / the partials and nothing else, the scan's destinations are global_load_dword.

One compile of the translation unit (about 100 s) is shared by the module."""
import collections
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("asm_load_waits", os.path.join(ROOT, "tools", "asm_load_waits.py"))
alw = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(alw)

X4, X1 = "global_load_dwordx4", "global_load_dword"


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    out = tmp_path_factory.mktemp("asm") / "sg.s"
    return open(alw.compile_listing(str(out))).read()


@pytest.fixture(scope="module")
def ev(listing):
    return alw.events(listing)


def runs(events):
    """the runs of a kernel: lists of load mnemonics, in program order"""
    out, run = [], []
    for what, x in events:
        if what == "load":
            run.append(x)
        elif what == "wait" and x < len(run):
            out.append(run); run = []
    if run:
        out.append(run)
    return out


def kernel(ev, part):
    names = [k for k in ev if part in k]
    assert len(names) == 1, (part, names)
    return ev[names[0]]


def test_runs_on_a_hand_written_stream():
    """the model itself: a counted wait that leaves the whole run in flight does not cut it, one that retires its oldest load does"""
    e = [("load", X1), ("load", X1), ("wait", 2), ("load", X4), ("wait", 2), ("load", X1), ("label", ".LBB0_1"), ("wait", 0), ("wait", 0), ("load", X4)]
    assert runs(e) == [[X1, X1, X4], [X1], [X4]]
    text = "_Z1kv:\n\tglobal_load_dword v1, v[2:3], off\n\ts_waitcnt vmcnt(0)\n.LBB0_1:\n\tglobal_load_dwordx4 v[4:7], v[2:3], off\n\tv_mov_b32 v0, v1\n" \
           "\tv_mov_b32 v0, v1\n\ts_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_waitcnt lgkmcnt(0)\n\ts_endpgm\n"
    assert alw.events(text) == {"_Z1kv": [("load", X1), ("wait", 0), ("label", ".LBB0_1"), ("load", X4), ("wait", 0)]}
    assert alw.census(text) == {"_Z1kv": (2, 1)}                      # (the second load's wait comes three instructions behind it)


def test_a_trip_of_the_new_scan_form_is_one_batch(ev):
    """all sixteen 16-byte loads of k3_in_part<1> (x and y of eight edges) lie in ONE run, together with the eight destination loads of
    the next trip: 24 loads, no wait among them that retires any"""
    r = runs(kernel(ev, "k3_in_partILi1EE"))
    with16 = [x for x in r if X4 in x]
    assert len(with16) == 1, [collections.Counter(x) for x in with16]
    c = collections.Counter(with16[0])
    assert c[X4] == 16 and c[X1] == 8 and sum(c.values()) == 24, c


def test_the_prologue_of_the_new_scan_form_is_one_batch(ev):
    """the run ahead of the trip's holds the eight destination loads of the first trip, and they are its last eight: none of them is
    retired before the eighth is issued"""
    r = runs(kernel(ev, "k3_in_partILi1EE"))
    trip = [i for i, x in enumerate(r) if X4 in x][0]
    assert trip >= 1 and len(r[trip - 1]) >= 8 and r[trip - 1][-8:] == [X1] * 8, r[max(0, trip - 2):trip]


def test_form_0_of_the_scan_is_what_the_check_is_for(ev, listing):
    """the same reading of k3_in_part<0>: whatever width its accumulator loads have, no run holds those of more than a few edges — each
    pair sits behind its own range test and is waited for there — and the census counts at least a dozen more drained loads than in
    form 1 (sixteen conditional loads a trip, eight ahead of the loop)"""
    r = runs(kernel(ev, "k3_in_partILi0EE"))
    wide = ("global_load_dwordx2", "global_load_dwordx3", X4)
    assert max(sum(1 for m in x if m in wide) for x in r) < 8, [collections.Counter(x) for x in r]
    cen = alw.census(listing)
    c0, c1 = ([v for k, v in cen.items() if part in k][0] for part in ("k3_in_partILi0EE", "k3_in_partILi1EE"))
    assert c1[1] <= c0[1] - 12, (c0, c1)


def test_the_slice_loads_of_the_eight_lane_features_are_whole_batches(ev):
    """k3_node_features_lanes: 24 16-byte loads (eight slices per lane, three words each) in one run for every 64 slices, 18 in one run for
    the last 48 or fewer.  The kernel's only other 16-byte load stands alone: the two alive counters its last thread re-arms"""
    r = runs(kernel(ev, "k3_node_features_lanes"))
    n16 = sorted(collections.Counter(x)[X4] for x in r if X4 in x)
    assert n16 == [1, 18, 24], n16
