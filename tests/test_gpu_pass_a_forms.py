"""Every form of K1 pass A on one small mixed trace: k1a_tile_partition (one and two sub-tiles), k1a_team_partition and k1a_partition
(with and without the histogram), level 2 of the join staged as u16, as u32 and read from global memory, unsharded and sharded.
The plan picks ONE pass-A kernel per engine, so the rest of the suite reaches a family only where a test's shape happens to ask for
it; here the development build's knobs name the form, geometry() confirms it ran, and the rows and drop counters must equal the
oracle's — and, across the narrow forms, one another byte for byte.

Two workgroups (SG_NWG=2) and 256 partitions: a team owns 4 units of at most 2048 events, so ~40 000 events in two unequal ingest
calls give every team several tiles per launch — tickets, the copy-out of the previous tile under the next one's loads, the first /
not-first header paths and the rotation of the units between launches."""
import os

import numpy as np
import pytest

from alaz_amd import replay, weights
from tests.helpers import CLOCK, HostShim, compare_edge_dicts, engine_edge_dict

pytestmark = pytest.mark.gpu

LAYERS = 1
MAX_LABELS = 64
SPLIT = 27_001                     # the two ingest calls: 27 001 events, then the rest
KNOBS = ("SG_NP", "SG_NWG", "SG_K1A", "SG_NSUB", "SG_L2_U32", "SG_L2_GLOBAL")


def _mixed_trace(topo, seed):
    """requests with raw outbound IPs, Host labels, non-pod sources, reversed events and mixed protocols; plain fast-path traffic;
    one hot key; open connections; durations of 2^32 ns and more; labels beyond the engine's label capacity"""
    ev, labels = replay.make_events(topo, 20_000, seed, mixed=True, with_raw_outbound=True, with_reverse=True)
    plain, _ = replay.make_events(topo, 12_000, seed + 1, stream_base=300)
    plain["host_label"] = 0                                          # (its own label numbering is not the first trace's: its outbound requests name raw IPs)
    rng = np.random.default_rng(seed + 2)
    hot = np.repeat(plain[:1], 5000)                                 # one edge, 5000 requests
    hot["saddr"] = topo.pod_ips[topo.edge_src[0]]; hot["daddr"] = topo.node_ip(topo.edge_dst[:1])[0]
    hot["duration_ns"] = rng.integers(1, 1 << 30, len(hot)); hot["status"] = np.where(rng.random(len(hot)) < 0.1, 503, 200)
    n_alive = 2000
    al = np.zeros(n_alive, dtype=replay.EVENT_DTYPE)
    al["flags"] = replay.EV_ALIVE
    al["saddr"] = topo.pod_ips[topo.edge_src[rng.integers(0, len(topo.edge_src), n_alive)]]
    kind = rng.random(n_alive)
    al["daddr"] = np.where(kind < 0.5, topo.svc_ips[rng.integers(0, topo.n_svcs, n_alive)],
                  np.where(kind < 0.8, topo.pod_ips[rng.integers(0, topo.n_pods, n_alive)],
                           0x5DB8D800 + rng.integers(0, 40, n_alive))).astype(np.uint32)
    al["saddr"][-30:] = 0xC0A80001                                   # not a pod: ignored, not counted
    al["host_label"][::7] = 1; al["flags"][::11] |= replay.EV_REVERSE; al["duration_ns"] = 12345; al["status"] = 503   # all ignored for open connections
    ev["duration_ns"][::401] = (1 << 32) + rng.integers(0, 1 << 33, len(ev["duration_ns"][::401]))
    hot["duration_ns"][::1250] = (1 << 32) | 7                       # ... and on a key the cache holds
    oor = np.repeat(plain[1:2], 9)                                   # Host labels beyond max_labels: dropped for capacity, counted
    oor["saddr"] = topo.pod_ips[topo.edge_src[:9]]; oor["daddr"] = replay.EXTERNAL_IP_BASE + 3; oor["host_label"] = MAX_LABELS + 3
    out = np.concatenate([ev[:9000], al[:900], hot[:2000], plain[:6000], oor[:4], ev[9000:], hot[2000:], al[900:], plain[6000:], oor[4:]])
    assert len(labels) <= MAX_LABELS and 38_000 < len(out) < 42_000
    return out, labels


def _oracle_window(topo, ev, labels):
    from oracle import pyoracle
    o = pyoracle.Oracle(*CLOCK); o.apply_ops(topo.k8s_ops())
    o.packed(ev, labels); o.window_close(weights.make_weights(LAYERS), LAYERS)
    return o


_CACHE = {}


def _case():
    """the trace, what the oracle makes of it (computed once) and the drops it does not model: labels out of range"""
    if "full" not in _CACHE:
        topo = replay.make_topology(150, 1500, seed=131)
        ev, labels = _mixed_trace(topo, 132)
        oor = ev["host_label"] > MAX_LABELS
        _CACHE["full"] = (topo, ev, labels, _oracle_window(topo, ev[~oor], labels), int(oor.sum()))
    return _CACHE["full"]


def _run(topo, ev, labels, knobs, **kw):
    from alaz_amd import engine
    for k in KNOBS: os.environ.pop(k, None)
    os.environ.update({"SG_NP": "256", "SG_NWG": "2"}, **knobs)
    try:
        g = engine.ServiceGraph(max_known_nodes=topo.n_nodes + 8, max_edges=8192, layers=LAYERS, max_labels=MAX_LABELS, max_outbound_ips=512,
                                max_window_events=1 << 16, dev_knobs=True, **kw)
        g.set_clock(*CLOCK); g.load_weights(weights.make_weights(LAYERS))
        shim = HostShim(); shim.apply(g, topo.k8s_ops())
        for part in (ev[:SPLIT], ev[SPLIT:]):
            while g.ingest(part) != 0:
                pass
        g.set_label_count(len(labels))
        rows = g.flush_window().copy()
        geo, st, ob = g.geometry(), g.stats(), g.outbound_ips().copy()
        g.close()
    finally:
        for k in KNOBS: os.environ.pop(k, None)
    assert geo["partitions"] == 256 and geo["pass_a_workgroups"] == 2, geo
    return rows, geo, st, shim, ob


def _check_against_oracle(rows, st, shim, ob, labels, o, n_oor, **kw):
    compare_edge_dicts(engine_edge_dict(rows, shim, labels, ob), o.edge_dict(), **kw)
    orow = o.edge_rows()
    assert np.array_equal(rows["from_ref"], orow["from_ref"]) and np.array_equal(rows["to_ref"], orow["to_ref"])
    assert st.last_window_events == o.window_events and st.events_dropped_src == o.dropped_src > 0
    assert st.events_misrouted == 0 and st.events_dropped_cap == n_oor > 0


FORMS = {"tile1": dict(SG_K1A="tile", SG_NSUB="1"), "tile2": dict(SG_K1A="tile", SG_NSUB="2"), "team": dict(SG_K1A="team")}
LEVEL2 = {"u16": ({}, 2), "u32": (dict(SG_L2_U32="1"), 1), "global": (dict(SG_L2_GLOBAL="1"), 0)}


def _assert_form(geo, form, l2_want):
    assert geo["k1_narrow"] == 1 and geo["join_l2_in_lds"] == l2_want, geo
    if form == "team": assert geo["pass_a_teams"] == 2 and geo["tile_records"] == 2048, geo
    else: assert geo["pass_a_teams"] == 0 and geo["tile_records"] == 4096 * int(form[-1]), geo


@pytest.mark.parametrize("l2", list(LEVEL2))
@pytest.mark.parametrize("form", list(FORMS))
def test_narrow_pass_a_forms_against_the_oracle_and_one_another(form, l2):
    topo, ev, labels, o, n_oor = _case()
    rows, geo, st, shim, ob = _run(topo, ev, labels, {**FORMS[form], **LEVEL2[l2][0]}, k1_variant=3, warm=False)
    _assert_form(geo, form, LEVEL2[l2][1])
    _check_against_oracle(rows, st, shim, ob, labels, o, n_oor)
    first = _CACHE.setdefault("narrow_rows", (rows.tobytes(), f"{form}-{l2}"))
    assert rows.tobytes() == first[0], f"the rows of {form}-{l2} differ from those of {first[1]}"


@pytest.mark.parametrize("hist", [False, True])
def test_wide_pass_a_against_the_oracle(hist):
    topo, ev, labels, o, n_oor = _case()
    rows, geo, st, shim, ob = _run(topo, ev, labels, {}, k1_variant=2, edge_histogram=hist)
    assert geo["k1_narrow"] == 0 and geo["pass_a_teams"] == 0 and geo["join_l2_in_lds"] == 1, geo
    _check_against_oracle(rows, st, shim, ob, labels, o, n_oor, percentiles=hist)


@pytest.mark.parametrize("form", ["tile2", "team"])
def test_sharded_pass_a_forms_on_one_shard_of_two(form):
    """SHARDED = true: rank 0 of 2 is fed the mixed trace of its shard view.  The reversed events whose from-endpoint (the service,
    label or raw IP they name as destination) another shard owns must be counted as misrouted; what is left must be the oracle's
    edges and integer accumulators on the events this shard owns.  (One shard alone has no halo exchange: its scores are not the
    oracle's, and an outbound IP that only misrouted events name still takes a slot, so identities are compared through the IPs.)"""
    from alaz_amd import sharded
    full = _case()[0]
    topo = sharded.shard_view(full, 0, 2)
    ev, labels = _mixed_trace(topo, 142)
    pod = {int(ip): i for i, ip in enumerate(topo.pod_ips)}; svc = {int(ip): topo.n_pods + j for j, ip in enumerate(topo.svc_ips)}
    src_pod = np.isin(ev["saddr"], topo.pod_ips)
    oor = ev["host_label"] > MAX_LABELS
    elsewhere = (sharded.route_events(ev, 2, pod, svc) != 0) & src_pod & ~oor
    o = _oracle_window(topo, ev[~oor & ~elsewhere], labels)
    rows, geo, st, shim, ob = _run(topo, ev, labels, FORMS[form], k1_variant=3, warm=False, rank=0, world=2)
    _assert_form(geo, form, 2)
    got, want = engine_edge_dict(rows, shim, labels, ob), o.edge_dict()
    assert set(got) == set(want)
    for k, w in want.items():
        assert got[k][:5] == w[:5] and got[k][8] == w[8], (k, got[k], w)
    assert st.last_window_events == o.window_events and st.events_dropped_src == o.dropped_src > 0
    assert st.events_misrouted == int(elsewhere.sum()) > 0 and st.events_dropped_cap == int(oor.sum()) > 0
