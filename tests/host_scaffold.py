"""What the CPU tests of the window stages share: windows built from tuples, K13's drifting edge sets and the GraphDS stand-in.  numpy,
the references and alaz_amd's Python only — no library, no GPU.  Not a test module: nothing here is collected, and asserts carry their
own messages (pytest rewrites asserts in test modules only).

rows_of exists once per shape of tuple the stages' tests write their windows in; a module imports its own as rows_of."""
import struct

import numpy as np

from alaz_amd import engine, hostlib
from alaz_amd.replay import EDGE_OUT_DTYPE
from tests.group_nodes_ref import group_nodes_ref
from tests.group_ref import group_ref
from tests.incident_ref import incident_ref
from tests.nodes_ref import nodes_ref

NEW, SPLIT, MERGED = engine.TRACK_NEW, engine.TRACK_SPLIT, engine.TRACK_MERGED
OBIP = 2 << 30
LABEL = 1 << 30


# ---- K13's constructed windows (tests/test_track_host.py; tests/test_group_track_host.py imports this module as k13) ----------------
def window_of(edges):
    """(node rows, incident per node row, incident rows) of a window whose red rows are exactly `edges`, (from_ref, to_ref) pairs"""
    edges = sorted(set(edges))
    r = np.zeros(len(edges), dtype=EDGE_OUT_DTYPE)
    for j, (f, t) in enumerate(edges):
        r[j]["from_ref"], r[j]["to_ref"], r[j]["score"] = f, t, 0.9
        r[j]["count"], r[j]["err_count"], r[j]["sum_ns"] = 10 + j, j % 3, 1000 * (j + 1)
    nodes = nodes_ref(r)
    inc, node_inc = incident_ref(r, nodes, "score", 0.5)
    return nodes, node_inc, inc


def chain(*ids):
    return list(zip(ids[:-1], ids[1:]))


def random_sequence(seed, windows=30, n_nodes=40):
    """edge sets that drift: a few edges die and a few are born per window, now and then a burst of deaths or an empty window; refs
    are pods, a few labels and a few outbound IPs (whose index means another address in every window)"""
    rng = np.random.default_rng(7000 + seed)
    refs = list(range(n_nodes - 6)) + [LABEL | k for k in range(3)] + [OBIP | k for k in range(3)]
    pods = n_nodes - 6
    alive = set()
    out = []
    for w in range(windows):
        mode = rng.random()
        if mode < 0.12:
            out.append([]); continue                                  # a silent window: the edges come back afterwards
        if mode < 0.22:
            alive = {e for e in alive if rng.random() < 0.3}
        alive = {e for e in alive if rng.random() < 0.8}
        for _ in range(int(rng.integers(2, 7))):
            a = int(rng.integers(0, pods))                            # (a pod at one end of every row)
            b = refs[int(rng.integers(0, len(refs)))]
            alive.add((a, b) if rng.random() < 0.8 or b >= LABEL else (b, a))
        out.append(sorted(alive))
    return out


def _coverage(ref_before, rows, ended, table_after, w, quiet):
    met = set()
    flags = rows["flags"]
    if (flags & MERGED).any():
        met.add("merged")
    old = {e["track"]: e for e in ref_before}
    for r in rows:
        if r["flags"] & SPLIT:
            claimant = [x for x in rows if x["track"] == r["parent"]]
            if claimant:
                met.add("split_kept" if claimant[0]["kept_nodes"] > r["kept_nodes"] else "split_tie")
        if not r["flags"] & NEW and old[r["track"]]["last_window"] < w - 1:
            met.add("revival")
    if len(ended):
        met.add("ended")
    now = {e["track"] for e in table_after}
    if any(t not in now for t in old):
        met.add("expiry")
    return met


# ---- rows from tuples ---------------------------------------------------------------------------------------------------------------
def trend_rows_of(*edges):
    """rows from (from_ref, to_ref, count, err_count, sum_ns) tuples"""
    r = np.zeros(len(edges), dtype=EDGE_OUT_DTYPE)
    for i, (f, t, c, e, s) in enumerate(edges):
        r[i]["from_ref"], r[i]["to_ref"], r[i]["count"], r[i]["err_count"], r[i]["sum_ns"] = f, t, c, e, s
    return r


def node_trend_rows_of(*edges):
    """canonical-order rows from (from_ref, to_ref, count, err_count, sum_ns) tuples (sorted here)"""
    r = np.zeros(len(edges), dtype=EDGE_OUT_DTYPE)
    for i, (f, t, c, e, s) in enumerate(sorted(edges)):
        r[i]["from_ref"], r[i]["to_ref"], r[i]["count"], r[i]["err_count"], r[i]["sum_ns"] = f, t, c, e, s
    return r


def rank_rows_of(*edges):
    """canonical-order rows from (from_ref, to_ref, score) tuples (sorted here), one request each"""
    r = np.zeros(len(edges), dtype=EDGE_OUT_DTYPE)
    for i, (f, t, s) in enumerate(sorted(edges)):
        r[i]["from_ref"], r[i]["to_ref"], r[i]["score"], r[i]["count"] = f, t, s, 1
    return r


def incident_rows_of(*edges):
    """canonical-order rows from (from_ref, to_ref, score) tuples (sorted here); count, err_count and sum_ns tell the rows apart"""
    r = np.zeros(len(edges), dtype=EDGE_OUT_DTYPE)
    for i, (f, t, s) in enumerate(sorted(edges, key=lambda e: (e[0], e[1]))):
        r[i]["from_ref"], r[i]["to_ref"], r[i]["score"] = f, t, s
        r[i]["count"], r[i]["err_count"], r[i]["sum_ns"] = 10 + i, i, 1000 * (i + 1)
    return r


def contract(rows, gmap, mg, mk, ml):
    ge, _, _ = group_ref(rows, np.asarray(gmap, np.uint32), mg, mk, ml)
    return ge, group_nodes_ref(ge, mg, mk, ml)


def _okey(x):
    """total order of float32 bit patterns: -0.0 below +0.0 (written apart from nodes_ref.score_key)"""
    b, = struct.unpack("<I", struct.pack("<f", x))
    return (1 << 31) + b if b < (1 << 31) else (1 << 32) - 1 - b


# ---- hostlib.GraphDS without an engine library: its mock records the calls it would make --------------------------------------------
def _ds():
    return hostlib.GraphDS(engine.make_config(max_known_nodes=64, max_edges=256), engine_lib=None)
