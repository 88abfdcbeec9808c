"""k1a_team_partition's paired form (sg_k1_team.h, PAIR = 1: a team sorts the two tiles it draws one behind the other into one LDS
tile and copies them out together) against the unpaired form and the oracle, on the development build: SG_K1A_PAIR=1 / =0 name the
form, geometry()["pass_a_pair"] confirms it.

Eight workgroups (SG_NWG=8) are 16 units; a tile is 2 048 events, and a team draws a second tile — a pair — only in a batch of more
than 16 full tiles (a smaller batch is cut into at most one shorter tile per unit), so 65 536 events are exactly one pair per team.
Rows (flush_window, ordered by (from_ref, to_ref)) must be equal byte for byte between the forms and equal to the oracle's; the
statistics counters must be equal too.  2 000 pods over 36 000 edges: 256 partitions, and 512 by SG_NP; 1 024 partitions are the
records ARRIVING SPLIT — one pass-B table of 2 048 slots per partition instead of two sub-tables (SG_NP=1024 SG_SPLIT=1 SG_HT=2048),
with the 512 cache slots a C3 engine has left beside pairs there (SG_CT)."""
import os

import numpy as np
import pytest

from alaz_amd import replay, weights
from tests.gpu_model_scaffold import MAX_LABELS, STATS, _CACHE, _on_edges, _sorted, _topo
from tests.helpers import CLOCK, HostShim, compare_edge_dicts, engine_edge_dict

pytestmark = pytest.mark.gpu

LAYERS = 1

UNITS, TILE = 16, 2048
KNOBS = ("SG_NP", "SG_NWG", "SG_K1A", "SG_K1A_PAIR", "SG_CT", "SG_SPLIT", "SG_HT")
SPLIT_KNOBS = dict(SG_SPLIT="1", SG_HT="2048", SG_CT="512")          # beside SG_NP=1024 (the cache a C3 engine has left there beside pairs)


def _oracle(key, ev):
    """the oracle's window for a trace, computed once per trace"""
    if ("oracle", key) not in _CACHE:
        from oracle import pyoracle
        topo, ops, _, _, labels = _topo()
        o = pyoracle.Oracle(*CLOCK); o.apply_ops(ops)
        o.packed(ev, labels); o.window_close(weights.make_weights(LAYERS), LAYERS)
        _CACHE[("oracle", key)] = o
    return _CACHE[("oracle", key)]


def _run_windows(windows, pair, np_=256, warm=False, rebuild=False, **knobs):
    """one engine over the windows (each a list of batches); per window (rows, counters), then the shim, the outbound IPs and the
    engine's last statistics.  warm: the engine keeps the edge set from window to window; rebuild: ... but sg_set_warm(0) makes it
    rebuild every window."""
    from alaz_amd import engine
    topo, ops, _, _, labels = _topo()
    for k in KNOBS: os.environ.pop(k, None)
    os.environ.update({"SG_NP": str(np_), "SG_NWG": "8", "SG_K1A": "team", "SG_K1A_PAIR": str(pair)}, **{**(SPLIT_KNOBS if np_ == 1024 else {}), **knobs})
    out = []
    try:
        g = engine.ServiceGraph(max_known_nodes=topo.n_nodes + 8, max_edges=65536, layers=LAYERS, max_labels=MAX_LABELS, max_outbound_ips=512,
                                max_window_events=1 << 18, dev_knobs=True, k1_variant=3, warm=warm)
        g.set_clock(*CLOCK); g.load_weights(weights.make_weights(LAYERS))
        if rebuild: g.set_warm(False)
        shim = HostShim(); shim.apply(g, ops)
        g.set_label_count(len(labels))
        for batches in windows:
            for part in batches:
                while g.ingest(part) != 0:
                    pass
            rows = _sorted(g.flush_window().copy())
            st = g.stats()
            out.append((rows, {k: int(getattr(st, k)) for k in STATS}, int(st.last_window_new_edges)))
        geo, st, ob = g.geometry(), g.stats(), g.outbound_ips().copy()
        g.close()
    finally:
        for k in KNOBS: os.environ.pop(k, None)
    assert geo["partitions"] == np_ and geo["pass_a_workgroups"] == 8 and geo["pass_a_teams"] == 2 and geo["tile_records"] == TILE, geo
    assert geo["pass_a_pair"] == pair and geo["k1_narrow"] == 1 and geo["warm_windows"] == int(warm), geo
    if np_ == 1024: assert geo["pass_b_split"] == 1 and geo["table_slots"] == 2048 and geo["cache_slots"] == 512, geo
    return out, shim, ob, st


def _run(batches, pair, np_=256, **knobs):
    out, shim, ob, _ = _run_windows([batches], pair, np_, **knobs)
    return out[0][0], out[0][1], shim, ob


def _both_forms(batches, np_=256, **knobs):
    """the two forms on the same batches: equal rows, byte for byte, and equal counters.  Returns the paired form's."""
    p = _run(batches, 1, np_, **knobs)
    u = _run(batches, 0, np_, **knobs)
    assert p[1] == u[1], (p[1], u[1])
    assert p[0].tobytes() == u[0].tobytes(), "the rows of the paired form differ from the unpaired form's"
    return p


def _check_oracle(res, o):
    rows, st, shim, ob = res
    labels = _topo()[4]
    compare_edge_dicts(engine_edge_dict(rows, shim, labels, ob), o.edge_dict())
    orow = o.edge_rows()
    assert np.array_equal(rows["from_ref"], orow["from_ref"]) and np.array_equal(rows["to_ref"], orow["to_ref"])
    assert st["last_window_events"] == o.window_events and st["events_dropped_src"] == o.dropped_src and st["events_dropped_cap"] == 0


@pytest.mark.parametrize("np_", [256, 512, 1024])
@pytest.mark.parametrize("n", [2 * UNITS * TILE, 3 * UNITS * TILE, 2 * UNITS * TILE + 1])
def test_pairs_whole_odd_and_with_a_one_record_second_half(n, np_):
    """exactly two tiles per team; three, so that the odd last tile leaves alone; two and one event: a one-record tile as some pair's
    second half (or a third tile alone).  The mixed trace: raw outbound IPs, Host labels, non-pod sources, reversed events."""
    ev = _topo()[2][:n]
    res = _both_forms([ev], np_)
    _check_oracle(res, _oracle(("mixed", n), ev))
    if np_ == 256: _CACHE[("rows", n)] = res[0].tobytes()


def test_batches_below_one_tile_per_unit():
    """5 000 events are ten tiles of 512: no unit draws a second tile, six units (one team of six workgroups) draw none; then a batch
    of 16 tiles of 1 536"""
    ev = _topo()[2]
    for n in (5000, 20_000 + 4000):
        part = ev[100_000:100_000 + n]
        _check_oracle(_both_forms([part]), _oracle(("small", n), part))


@pytest.mark.parametrize("np_", [256, 1024])
def test_one_window_fed_as_seven_uneven_batches(np_):
    """k1a_rot, the ticket base and the piece counters carry across launches — pairs in some, single short tiles in others: the same rows
    as the same events in one batch"""
    n = 3 * UNITS * TILE
    ev = _topo()[2][:n]
    cuts = [0, 3000, 3001, 10_000, 10_000 + 2 * UNITS * TILE, 80_000, 97_000, n]
    assert len(cuts) == 8 and cuts == sorted(cuts)
    res = _both_forms([ev[a:b] for a, b in zip(cuts, cuts[1:])], np_)
    _check_oracle(res, _oracle(("mixed", n), ev))
    if np_ == 256 and ("rows", n) in _CACHE:
        assert res[0].tobytes() == _CACHE[("rows", n)]


def _kmix_partition(cf, ct, nb, pb):
    """sg_hash.h sg_kmix: the partition of the edge (cf, ct) of compact indices"""
    m = (1 << nb) - 1
    f = lambda v, c: (((v & 0xFFFFFF) * c) >> 8) & m
    l, r = cf, ct
    r ^= f(l, 0x9E3779); l ^= f(r, 0x85EBCB); r ^= f(l, 0xC2B2AF)
    return l >> (nb - pb)


def _hot_trace(n_hot):
    """every topology edge but three ONCE (16 full tiles: each team's first tile, which fills the smallest cache — 64 slots, SG_CT — with
    keys seen once, so that whatever is cached leaves as one narrow record like a record that travelled), then n_hot events on three
    edges of one partition, which then find no free cache slot and travel: runs of up to 2 048 records for one piece"""
    topo, _, _, plain, _ = _topo()
    nb = 12
    while (1 << nb) < topo.n_nodes + 8 + MAX_LABELS + 1024: nb += 1                        # sg_plan.hpp: known + labels + 2 x outbound IPs, at least 12 bits
    part = np.array([_kmix_partition(int(s), int(d), nb, 8) for s, d in zip(topo.edge_src, topo.edge_dst)])
    hot_e = np.flatnonzero(part == part[0])[:3]
    assert len(hot_e) == 3
    rest = np.setdiff1d(np.arange(len(topo.edge_src)), hot_e)[:UNITS * TILE]
    assert len(rest) == UNITS * TILE
    rng = np.random.default_rng(77)
    return np.concatenate([_on_edges(rest, rng), _on_edges(hot_e[rng.integers(0, 3, n_hot)], rng)]), nb


def test_a_combined_run_beyond_the_piece_goes_to_the_overflow_list():
    ev, _ = _hot_trace(3 * UNITS * TILE // 2)
    res = _both_forms([ev], SG_CT="64")
    _check_oracle(res, _oracle(("hot", len(ev)), ev))
    assert int(res[0]["count"].max()) > 10_000                        # the hot edges are whole: nothing was lost on the way through the list


def test_beyond_the_overflow_list_the_forms_drop_the_same_number():
    """more records for one partition than its eight pieces and the window's overflow list (65 536 entries) hold: every piece and the list
    fill up whichever form runs, and the count of dropped events — what is offered less what fits — must be the unpaired form's own"""
    ev, _ = _hot_trace(100_000)
    p = _run([ev], 1, SG_CT="64")
    u = _run([ev], 0, SG_CT="64")
    # (WHICH records are dropped follows the order the workgroups reach the list in, and a dropped record may be an edge's only one: the
    # rows and the edge / node counts are not compared, in either form they differ from run to run)
    for d in (p[1], u[1]): d.pop("last_window_edges"); d.pop("last_window_nodes")
    assert p[1] == u[1], (p[1], u[1])
    assert 0 < p[1]["events_dropped_cap"] < 100_000 - 65_536 and p[1]["last_window_events"] == u[1]["last_window_events"]


def _rare_trace(where):
    """65 536 fast-path events — the first 32 768 are every team's first tile (A), the rest the second tiles (B) — with rare events in
    A only, in B only or in both: open connections, raw outbound IPs, the IP in both maps, durations of 2^32 ns and more.  One hot
    edge runs through the whole trace: claimed in the cache during A, folded during B."""
    topo, _, _, plain, _ = _topo()
    n = 2 * UNITS * TILE
    ev = plain[:n].copy()
    rng = np.random.default_rng(55 + len(where))
    hot = np.arange(5, n, 97)
    ev["flags"][hot] = 0; ev["host_label"][hot] = 0
    ev["saddr"][hot] = topo.pod_ips[topo.edge_src[0]]; ev["daddr"][hot] = topo.node_ip(topo.edge_dst[:1])[0]
    halves = {"a": [(0, n // 2)], "b": [(n // 2, n)], "both": [(0, n // 2), (n // 2, n)]}[where]
    for lo, hi in halves:
        at = lo + rng.choice(hi - lo, 800, replace=False)
        at = at[~np.isin(at, hot)]
        k = np.arange(len(at)) % 4
        a = at[k == 0]                                                    # open connections
        ev["flags"][a] = replay.EV_ALIVE; ev["saddr"][a] = topo.pod_ips[topo.edge_src[a % len(topo.edge_src)]]
        a = at[k == 1]                                                    # raw outbound IPs
        ev["flags"][a] = 0; ev["host_label"][a] = 0; ev["daddr"][a] = 0x5DB8D800 + (a % 40); ev["saddr"][a] = topo.pod_ips[topo.edge_src[a % len(topo.edge_src)]]
        a = at[k == 2]                                                    # the IP that is a pod's and a service's
        ev["flags"][a] = 0; ev["daddr"][a] = topo.pod_ips[1]; ev["saddr"][a] = topo.pod_ips[topo.edge_src[a % len(topo.edge_src)]]
        a = at[k == 3]                                                    # 2^32 ns and more
        ev["duration_ns"][a] = (1 << 32) + rng.integers(0, 1 << 33, len(a))
        ev["duration_ns"][hot[(hot >= lo) & (hot < hi)][::9]] = (1 << 32) | 7   # ... also on the key the cache holds
    return ev


@pytest.mark.parametrize("where,np_", [("a", 256), ("b", 256), ("both", 256), ("both", 512), ("a", 1024), ("b", 1024), ("both", 1024)])
def test_rare_events_in_either_half_of_a_pair(where, np_):
    ev = _rare_trace(where)
    res = _both_forms([ev], np_)
    o = _oracle(("rare", where), ev)
    _check_oracle(res, o)


def test_arriving_split_through_a_warm_engine_three_windows():
    """1 024 partitions arriving split, paired, on an engine that keeps the edge set: 30 000 edges, the same and 50 new ones, the same
    again — a cold window, a delta window, a warm window, each of one pair per team.  Rows equal to those of an engine that rebuilds
    every window (sg_set_warm(0)) and to the oracle's."""
    from oracle import pyoracle
    topo, ops, _, _, labels = _topo()
    rng = np.random.default_rng(91)
    n, base, new = 2 * UNITS * TILE, 30_000, 50
    e1 = rng.integers(0, base, n); e1[:base] = np.arange(base)                 # every edge of the base set at least once
    e2 = np.concatenate([rng.integers(0, base, n - new), np.arange(base, base + new)]); e2[:base] = np.arange(base)
    e3 = rng.integers(0, base + new, n); e3[:base + new] = np.arange(base + new)
    windows = [[_on_edges(e, rng)] for e in (e1, rng.permutation(e2), e3)]
    warm, shim, ob, st = _run_windows(windows, 1, 1024, warm=True)
    cold, _, _, stc = _run_windows(windows, 1, 1024, warm=True, rebuild=True)
    assert (st.windows_cold, st.windows_warm, st.windows_delta) == (1, 2, 1) and warm[1][2] == new, (st.windows_cold, st.windows_warm, st.windows_delta, warm[1][2])
    assert stc.windows_warm == 0
    o = pyoracle.Oracle(*CLOCK); o.apply_ops(ops)
    for (rows, counters, _), (crows, ccounters, _), w in zip(warm, cold, windows):
        assert rows.tobytes() == crows.tobytes() and counters == ccounters
        o.packed(w[0], labels); o.window_close(weights.make_weights(LAYERS), LAYERS)
        _check_oracle((rows, counters, shim, ob), o)
