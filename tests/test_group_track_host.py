"""K19, the workload tracks, on the CPU: the reference tests/group_track_ref.py against K13's (tests/track_ref.py) where no ref is a
group's, against a second formulation written apart from it (every track owns a set of refs) over random sequences of windows that
mix group, known, label and outbound-IP refs, hand-written known answers for every rule of the contract, and the plan in
alaz_amd/csrc/sg_plan.hpp (tests/micro/plan_driver.cpp, stage group_track)."""
import os

import numpy as np
import pytest

from alaz_amd import engine
from tests.group_incident_ref import group_incident_ref
from tests.group_nodes_ref import group_nodes_ref
from tests.group_track_ref import GroupTrackRef, is_group_anchor
from tests import host_scaffold as k13
from tests.plan_driver import plan_fixture
from tests.plan_layout import check_layout
from tests.track_ref import TrackRef

HERE = os.path.dirname(os.path.abspath(__file__))
NO = engine.NO_TRACK
NEW, SPLIT, MERGED = engine.TRACK_NEW, engine.TRACK_SPLIT, engine.TRACK_MERGED
LABEL, OBIP, GROUP = 1 << 30, 2 << 30, 3 << 30
MG, MK, ML = 32, 64, 8                                                # the id spaces of the constructed windows


def G(g):
    return GROUP | g


def window_of(edges):
    """(workload rows, incident per workload row, workload incident rows) of a window whose red group edges are exactly `edges`,
    (from_ref, to_ref) pairs"""
    edges = sorted(set(edges))
    ge = np.zeros(len(edges), dtype=engine.GROUP_EDGE_DTYPE)
    for j, (f, t) in enumerate(edges):
        ge[j]["from_ref"], ge[j]["to_ref"], ge[j]["score_max"] = f, t, 0.9
        ge[j]["count"], ge[j]["err_count"], ge[j]["sum_ns"], ge[j]["edges"] = 10 + j, j % 3, 1000 * (j + 1), 1
    gn = group_nodes_ref(ge, MG, MK, ML)
    inc, node_inc = group_incident_ref(ge, gn, "score", 0.5)
    return gn, node_inc, inc


chain = k13.chain


# ---- the contract again, on its own: every track owns the refs that were last seen in it -----------------------------------------------
class GroupTrackSets:
    def __init__(self, quiet, cap):
        self.quiet, self.cap, self.w, self.issued, self.cut = quiet, cap, 0, 0, 0
        self.tracks = []                                              # dict(id, parent, first, last, windows, peak, count, err, refs {ref: window})

    def step(self, nodes, node_inc, incidents):
        w = self.w
        owner = {ref: t["id"] for t in self.tracks for ref, seen in t["refs"].items() if w - seen <= self.quiet + 1}
        groups = [[] for _ in incidents]
        for v, i in enumerate(node_inc):
            ref = int(nodes["ref"][v])
            if i != engine.NO_INCIDENT and ref >> 30 != 2:              # everything but an outbound IP anchors
                groups[int(i)].append(ref)
        facts = []
        for i, refs in enumerate(groups):
            touched = sorted({owner[r] for r in refs if r in owner})
            oldest = touched[0] if touched else None
            facts.append(dict(i=i, oldest=oldest, kept=sum(1 for r in refs if oldest is not None and owner.get(r) == oldest),
                              moved=sum(1 for r in refs if r in owner and owner[r] != oldest), joined=sum(1 for r in refs if r not in owner)))
        winner = {}
        for t in self.tracks:
            rivals = sorted((f for f in facts if f["oldest"] == t["id"]), key=lambda f: (-f["kept"], f["i"]))
            if rivals:
                winner[t["id"]] = rivals[0]["i"]
        fresh = [f for f in facts if f["oldest"] is None or winner[f["oldest"]] != f["i"]]
        ended = [dict(t) for t in self.tracks if t["id"] not in winner and t["last"] == w - 1]
        born = {}
        for n, f in enumerate(fresh):
            o = incidents[f["i"]]
            born[f["i"]] = dict(id=self.issued + n, parent=NO if f["oldest"] is None else f["oldest"], first=w, last=w, windows=1,
                                peak=int(o["nodes"]), count=int(o["count"]), err=int(o["err"]), refs={})
        self.issued += len(fresh)
        for t in self.tracks:
            if t["id"] in winner:
                o = incidents[winner[t["id"]]]
                t.update(last=w, windows=t["windows"] + 1, peak=max(t["peak"], int(o["nodes"])), count=(t["count"] + int(o["count"])) % 2 ** 64,
                         err=(t["err"] + int(o["err"])) % 2 ** 64)
        by_id = {t["id"]: t for t in self.tracks}
        rows = np.zeros(len(incidents), dtype=engine.TRACK_DTYPE)
        for f in facts:
            t = born.get(f["i"]) or by_id[f["oldest"]]
            flags = (MERGED if f["moved"] else 0) | (NEW if f["i"] in born else 0) | (SPLIT if f["i"] in born and f["oldest"] is not None else 0)
            rows[f["i"]] = (t["id"], t["parent"], t["first"], t["windows"], f["kept"], f["moved"], f["joined"], flags)
            for r in groups[f["i"]]:
                for other in self.tracks:
                    other["refs"].pop(r, None)
                t["refs"][r] = w
        keep = [t for t in self.tracks if t["id"] in winner or w - t["last"] <= self.quiet] + [born[i] for i in sorted(born)]
        self.cut += max(0, len(keep) - self.cap)
        self.tracks = keep[: self.cap]
        self.w += 1
        return rows, self._arr(ended)

    @staticmethod
    def _arr(ts):
        out = np.zeros(len(ts), dtype=engine.TRACK_ENTRY_DTYPE)
        for k, t in enumerate(ts):
            out[k] = (t["id"], t["parent"], t["first"], t["last"], t["windows"], t["peak"], t["count"], t["err"])
        return out

    def entries(self):
        return self._arr(self.tracks)


def random_sequence(seed, windows=30):
    """group edge sets that drift as tests/test_track_host.py's do; the refs are workloads, ungrouped pods, labels and outbound IPs (a
    group edge has a workload or a pod at one end), and now and then a pod changes sides: a workload's edges reappear under a pod's
    ref, or the other way round"""
    rng = np.random.default_rng(9100 + seed)
    near = [G(k) for k in range(12)] + list(range(20, 40))             # workloads and ungrouped pods
    far = near + [LABEL | k for k in range(3)] + [OBIP | k for k in range(3)]
    alive, out = set(), []
    for w in range(windows):
        mode = rng.random()
        if mode < 0.12:
            out.append([]); continue
        if mode < 0.22:
            alive = {e for e in alive if rng.random() < 0.3}
        if mode > 0.9 and alive:                                      # a regrouping: workload k's edges move to pod 20 + k, or back
            k = int(rng.integers(0, 12))
            a, b = (G(k), 20 + k) if rng.random() < 0.5 else (20 + k, G(k))
            alive = {(b if f == a else f, b if t == a else t) for f, t in alive}
        alive = {e for e in alive if rng.random() < 0.8}
        for _ in range(int(rng.integers(2, 7))):
            a = near[int(rng.integers(0, len(near)))]
            b = far[int(rng.integers(0, len(far)))]
            alive.add((a, b) if rng.random() < 0.8 or b >> 30 in (1, 2) else (b, a))
        out.append(sorted(alive))
    return out


def test_it_is_k13s_reference_where_no_ref_is_a_groups():
    for quiet in (0, 1, 3):
        for seed in range(6):
            a, b = TrackRef(quiet, 0, ncap=64), GroupTrackRef(quiet, 0, ncap=64)
            for w, edges in enumerate(k13.random_sequence(seed)):
                win = k13.window_of(edges)
                (r1, e1), (r2, e2) = a.step(*win), b.step(*win)
                assert r1.tobytes() == r2.tobytes() and e1.tobytes() == e2.tobytes(), (quiet, seed, w)
                assert a.entries().tobytes() == b.entries().tobytes() and a.stats() == b.stats()
    a, b = TrackRef(1, 3), GroupTrackRef(1, 3)                        # ... and where the table is cut
    for edges in k13.random_sequence(0):
        win = k13.window_of(edges)
        (r1, e1), (r2, e2) = a.step(*win), b.step(*win)
        assert r1.tobytes() == r2.tobytes() and e1.tobytes() == e2.tobytes() and a.stats() == b.stats()
    assert a.stats()["dropped_cap"] > 0


@pytest.mark.parametrize("quiet", [0, 1, 2])
def test_reference_against_the_sets_formulation(quiet):
    met, types_seen = set(), set()
    for seed in range(12):
        ref, sets = GroupTrackRef(quiet, 0, ncap=64), GroupTrackSets(quiet, (quiet + 1) * 64)
        for w, edges in enumerate(random_sequence(seed)):
            win = window_of(edges)
            before = ref.entries()
            rows, ended = ref.step(*win)
            rows2, ended2 = sets.step(*win)
            assert rows.tobytes() == rows2.tobytes(), (seed, w)
            assert ended.tobytes() == ended2.tobytes(), (seed, w)
            assert ref.entries().tobytes() == sets.entries().tobytes(), (seed, w)
            met |= k13._coverage(before, rows, ended, ref.entries(), w, quiet)
            types_seen |= set((win[0]["ref"][win[1] != engine.NO_INCIDENT] >> 30).tolist())
        assert ref.stats() == dict(windows=30, live=len(sets.tracks), opened=sets.issued, dropped_cap=0)
    assert types_seen == {0, 1, 2, 3}
    want = {"merged", "split_kept", "ended", "expiry"} | ({"revival"} if quiet else set())
    assert want <= met, want - met


def test_a_small_table_cuts_in_the_random_sequences():
    cuts = 0
    for seed in range(8):
        ref, sets = GroupTrackRef(1, 3), GroupTrackSets(1, 3)
        for w, edges in enumerate(random_sequence(seed)):
            win = window_of(edges)
            rows, ended = ref.step(*win)
            rows2, ended2 = sets.step(*win)
            assert rows.tobytes() == rows2.tobytes() and ended.tobytes() == ended2.tobytes(), (seed, w)
            assert ref.entries().tobytes() == sets.entries().tobytes() and len(ref.entries()) <= 3
        assert ref.stats()["dropped_cap"] == sets.cut
        cuts += sets.cut
    assert cuts > 0


# ---- known answers, one rule each, over workloads ---------------------------------------------------------------------------------------
def test_an_incident_that_stays_keeps_its_track():
    ref = GroupTrackRef(2, 0, ncap=16)
    for w in range(3):
        win = window_of(chain(G(1), G(2), 40))
        rows, ended = ref.step(*win)
        assert len(rows) == 1 and len(ended) == 0
        r = rows[0]
        assert (r["track"], r["parent"], r["first_window"], r["windows"]) == (0, NO, 0, w + 1)
        assert (r["kept_nodes"], r["moved_nodes"], r["joined_nodes"], r["flags"]) == ((0, 0, 3, NEW) if w == 0 else (3, 0, 0, 0))
    e, inc = ref.entries(), win[2][0]
    assert len(e) == 1 and (e[0]["track"], e[0]["first_window"], e[0]["last_window"], e[0]["windows"], e[0]["peak_nodes"]) == (0, 0, 2, 3, 3)
    assert e[0]["count"] == 3 * int(inc["count"]) and e[0]["err"] == 3 * int(inc["err"])
    assert ref.stats() == dict(windows=3, live=1, opened=1, dropped_cap=0)


def test_a_merge_continues_as_the_older_track_and_ends_the_younger():
    ref = GroupTrackRef(2, 0, ncap=16)
    rows, _ = ref.step(*window_of(chain(G(1), G(2)) + chain(G(5), G(6))))
    assert rows["track"].tolist() == [0, 1] and rows["flags"].tolist() == [NEW, NEW]
    young = ref.entries()[1]
    rows, ended = ref.step(*window_of(chain(G(1), G(2), G(5), G(6), G(7))))
    r = rows[0]
    assert len(rows) == 1 and (r["track"], r["windows"], r["kept_nodes"], r["moved_nodes"], r["joined_nodes"], r["flags"]) == (0, 2, 2, 2, 1, MERGED)
    assert len(ended) == 1 and ended.tobytes() == young.tobytes() and ended[0]["track"] == 1
    assert ref.entries()["track"].tolist() == [0, 1]
    rows, ended = ref.step(*window_of(chain(G(1), G(2), G(5), G(6), G(7))))
    assert (rows[0]["track"], rows[0]["kept_nodes"], rows[0]["moved_nodes"], rows[0]["flags"]) == (0, 5, 0, 0) and len(ended) == 0


@pytest.mark.parametrize("cut,first,second", [(4, (1, 0, 4, NEW | SPLIT), (0, NO, 6, 0)), (5, (0, NO, 5, 0), (1, 0, 5, NEW | SPLIT))])
def test_a_split_continues_in_the_piece_that_kept_most(cut, first, second):
    """workloads 1..10 cut into 1..cut and cut+1..10: 4 / 6 goes to the larger piece although it is the later incident, 5 / 5 to the first"""
    ref = GroupTrackRef(2, 0, ncap=16)
    ids = [G(k) for k in range(1, 11)]
    ref.step(*window_of(chain(*ids)))
    rows, ended = ref.step(*window_of(chain(*ids[:cut]) + chain(*ids[cut:])))
    assert len(rows) == 2 and len(ended) == 0
    for r, (track, parent, kept, flags) in zip(rows, (first, second)):
        assert (r["track"], r["parent"], r["kept_nodes"], r["moved_nodes"], r["joined_nodes"], r["flags"]) == (track, parent, kept, 0, 0, flags)
    e = ref.entries()
    assert e["track"].tolist() == [0, 1] and e["parent"].tolist() == [NO, 0] and e["peak_nodes"].tolist() == [10, cut]


@pytest.mark.parametrize("quiet", [0, 1, 2])
def test_a_flap_keeps_its_id_inside_the_quiet_span_and_expires_after_it(quiet):
    ref = GroupTrackRef(quiet, 0, ncap=16)
    c = chain(G(1), G(2), 33)
    ref.step(*window_of(c))
    listed = 0
    for _ in range(quiet):
        rows, ended = ref.step(*window_of([]))
        listed += len(ended)
        assert len(rows) == 0 and ref.entries()["track"].tolist() == [0]
    rows, ended = ref.step(*window_of(c))
    listed += len(ended)
    assert (rows[0]["track"], rows[0]["windows"], rows[0]["kept_nodes"], rows[0]["flags"]) == (0, 2, 3, 0)
    assert listed == (1 if quiet else 0)
    for k in range(quiet + 1):                                        # one silent window more than it survives
        rows, ended = ref.step(*window_of([]))
        assert len(ended) == (1 if k == 0 else 0)
        assert ref.entries()["track"].tolist() == ([0] if k < quiet else [])
    rows, ended = ref.step(*window_of(c))
    assert (rows[0]["track"], rows[0]["parent"], rows[0]["windows"], rows[0]["joined_nodes"], rows[0]["flags"]) == (1, NO, 1, 3, NEW)


def test_an_outbound_ip_never_anchors_and_a_group_ref_does():
    ref = GroupTrackRef(2, 0, ncap=16)
    win = window_of([(G(1), OBIP | 0)])
    rows, _ = ref.step(*win)
    assert win[2]["nodes"][0] == 2 and (rows[0]["track"], rows[0]["joined_nodes"], rows[0]["kept_nodes"]) == (0, 1, 0)
    rows, _ = ref.step(*window_of([(G(2), OBIP | 0)]))                # the same index is another address now
    assert (rows[0]["track"], rows[0]["parent"], rows[0]["joined_nodes"], rows[0]["kept_nodes"], rows[0]["flags"]) == (1, NO, 1, 0, NEW)
    rows, _ = ref.step(*window_of([(G(1), OBIP | 5)]))                # the workload carries its track to whatever address it calls
    assert (rows[0]["track"], rows[0]["kept_nodes"], rows[0]["flags"]) == (0, 1, 0)
    rows, _ = ref.step(*window_of([(G(3), LABEL | 4)]))
    rows, _ = ref.step(*window_of([(G(4), LABEL | 4)]))               # a label is an anchor
    assert (rows[0]["track"], rows[0]["kept_nodes"], rows[0]["joined_nodes"], rows[0]["flags"]) == (2, 1, 1, 0)
    assert all(is_group_anchor(r) for r in (G(0), G(MG - 1), 7, LABEL | 4)) and not is_group_anchor(OBIP | 0)
    # group g and pod g are two anchors: the pod's incident does not continue the group's
    ref = GroupTrackRef(2, 0, ncap=16)
    ref.step(*window_of([(G(7), G(8))]))
    rows, _ = ref.step(*window_of([(7, 8)]))
    assert (rows[0]["track"], rows[0]["parent"], rows[0]["joined_nodes"], rows[0]["flags"]) == (1, NO, 2, NEW)


@pytest.mark.parametrize("gap", [0, 1])
def test_a_pod_regrouped_between_windows_leaves_its_old_member_to_age_out(gap):
    """quiet 1.  Window 0: workload 2 (pod 25 among its pods) calls pod 40: track 0.  Window 1: pod 25 has left the workload and calls
    pod 40 under its own ref: pod 40's member carries track 0 on, and pod 25 JOINS — workload 2's member did not move with it.  That
    member stays with workload 2's key: the workload back in window 2 is kept by track 0, back in window 3 it has aged out"""
    ref = GroupTrackRef(1, 0, ncap=16)
    rows, _ = ref.step(*window_of([(G(2), 40)]))
    assert (rows[0]["track"], rows[0]["joined_nodes"]) == (0, 2)
    rows, _ = ref.step(*window_of([(25, 40)]))
    assert (rows[0]["track"], rows[0]["kept_nodes"], rows[0]["joined_nodes"], rows[0]["moved_nodes"], rows[0]["flags"]) == (0, 1, 1, 0, 0)
    assert ref.member[G(2)] == (0, 0) and ref.member[25] == (0, 1)     # nothing migrated
    for _ in range(gap):
        ref.step(*window_of([(25, 40)]))
    rows, _ = ref.step(*window_of([(G(2), 41)]))
    r = rows[0]
    if gap == 0:
        assert (r["track"], r["kept_nodes"], r["joined_nodes"], r["flags"]) == (0, 1, 1, 0)
    else:
        assert (r["track"], r["parent"], r["kept_nodes"], r["joined_nodes"], r["flags"]) == (1, NO, 0, 2, NEW)


def test_the_table_is_cut_at_max_tracks():
    ref = GroupTrackRef(2, 2)
    pairs = chain(G(1), G(2)) + chain(G(3), G(4)) + chain(G(5), 36) + chain(37, 38)
    rows, _ = ref.step(*window_of(pairs))
    assert rows["track"].tolist() == [0, 1, 2, 3] and ref.entries()["track"].tolist() == [0, 1]
    assert ref.stats() == dict(windows=1, live=2, opened=4, dropped_cap=2)
    rows, ended = ref.step(*window_of(pairs))                          # a member that names an id the table lacks is not live
    assert rows["track"].tolist() == [0, 1, 4, 5] and rows["flags"].tolist() == [0, 0, NEW, NEW] and rows["parent"].tolist() == [NO] * 4
    assert rows["joined_nodes"].tolist() == [0, 0, 2, 2] and len(ended) == 0
    assert ref.entries()["track"].tolist() == [0, 1] and ref.stats() == dict(windows=2, live=2, opened=6, dropped_cap=4)


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------
plan = plan_fixture("group_track")


def _p(mg, mk, ml, nc, slots=1, ss=16, quiet=2, mt=0, res=0):
    return (mg, mk, ml, nc, slots, ss, quiet, mt, res)


# (max_groups, max_known, max_labels, nc): toy, config 3 (nc = min(GK, 2 x max_edges)), a large shard, the smallest, nothing
ENGINES = [(1024, 1024, 16, 2124), (12_000, 12_000, 1000, 27_000), (380_000, 380_000, 4000, 780_000), (1, 1, 0, 2), (0, 0, 0, 0)]


def test_plan_sizes(plan):
    for r in plan([_p(mg, mk, ml, nc, slots, quiet=q, mt=mt) for mg, mk, ml, nc in ENGINES for slots in (1, 3) for q in (0, 2, 15) for mt in (0, 8, 100_000)]):
        assert r["rc"] == 0 and r["ncap"] == r["nc"]
        nc, slots, mt = max(r["nc"], 1), r["slots"], r["max_tracks"]
        assert mt in (8, 100_000) or mt == (r["quiet"] + 1) * nc       # max_tracks 0 = (quiet_windows + 1) * nc
        span = max(nc, mt)
        assert r["per"] % 256 == 0 and 1 <= r["wgs"] <= 1024 and r["wgs"] * r["per"] >= span > (r["wgs"] - 1) * r["per"]
        assert 1 <= r["init_wgs"] <= 1024 and r["node_wgs"] == min(1024, -(-nc // 256)) and r["fold_wgs"] == min(1024, -(-nc // 2048))
        anchors = r["max_groups"] + r["max_known"] + r["max_labels"]
        assert r["anchors"] == anchors and r["member_bytes"] >= 4 * anchors
        assert r["table_bytes"] >= 40 * mt and r["claim_bytes"] >= 8 * mt and r["inc_bytes"] >= 4 * nc and r["state_bytes"] >= 24
        assert r["blk_bytes"] >= 7 * 1024 * 4 and r["rows_bytes"] >= 32 * nc and r["ended_bytes"] >= 40 * nc and r["count_bytes"] >= 8
        for k in ("member_bytes", "table_bytes", "state_bytes", "inc_bytes", "claim_bytes", "blk_bytes", "rows_bytes", "ended_bytes", "count_bytes"):
            assert r[k] % 256 == 0
        assert r["total_bytes"] == (2 * r["member_bytes"] + 2 * r["table_bytes"] + 2 * r["state_bytes"] + 6 * r["inc_bytes"] + r["claim_bytes"]
                                    + r["blk_bytes"] + slots * (r["rows_bytes"] + r["ended_bytes"] + r["count_bytes"]))
        # every piece 256-byte aligned, back to back (no two overlap), each at least what the kernels write, the slots' region last
        check_layout(r, {"mtrack": 4 * anchors, "mlast": 4 * anchors, "table0": 40 * mt, "table1": 40 * mt, "state0": 24, "state1": 24,
                         **{k: 4 * nc for k in ("cand", "kept", "moved", "joined", "pos", "tv")}, "claim": 8 * mt, "blk": 7 * 1024 * 4,
                         "rows": 32 * nc, "ended": 40 * nc, "ended_count": 8}, per_slot=("rows", "ended", "ended_count"))
        assert r["total_bytes"] <= 8 * anchors + 88 * mt + (24 + 72 * slots) * nc + 7 * 4096 + 256 * (14 + 3 * slots)
    c3, = plan([_p(12_000, 12_000, 1000, 27_000)])
    assert (c3["max_tracks"], c3["node_wgs"], c3["fold_wgs"]) == (81_000, 106, 14) and c3["total_bytes"] < 12 << 20


def test_the_anchor_count_does_not_wrap_at_two_to_the_thirty_groups(plan):
    r, = plan([_p(1 << 30, 12_000, 1000, 27_000)])
    anchors = (1 << 30) + 13_000
    assert r["rc"] == 0 and r["anchors"] == anchors
    assert r["member_bytes"] >= 4 * anchors > 1 << 32                  # one member array alone is past 4 GiB: sized in 64 bits
    lay = {n: (o, b) for n, o, b in r["layout"]}
    assert lay["mtrack"] == (0, r["member_bytes"]) and lay["mlast"][0] == r["member_bytes"] and lay["table0"][0] == 2 * r["member_bytes"]
    assert r["total_bytes"] > 2 * r["member_bytes"] > 1 << 33
    check_layout(r, {"mtrack": 4 * anchors, "mlast": 4 * anchors, "table0": 0, "table1": 0, "state0": 24, "state1": 24,
                     **{k: 0 for k in ("cand", "kept", "moved", "joined", "pos", "tv")}, "claim": 0, "blk": 0, "rows": 0, "ended": 0,
                     "ended_count": 8}, per_slot=("rows", "ended", "ended_count"))


def test_plan_parameter_checks(plan):
    """check_tracks over nc: K13's refusals"""
    ok = plan([_p(64, 1000, 10, 100, quiet=q) for q in (0, 1, 15)])
    assert [r["rc"] for r in ok] == [0] * 3 and [r["max_tracks"] for r in ok] == [100, 200, 1600]
    assert plan([_p(64, 1000, 10, 100, mt=7)])[0]["max_tracks"] == 7
    bad = plan([_p(64, 1000, 10, 100, quiet=16), _p(64, 1000, 10, 100, ss=12), _p(64, 1000, 10, 100, ss=20), _p(64, 1000, 10, 100, res=1),
                _p(64, 1000, 10, 1 << 28, quiet=15)])
    assert [r["rc"] for r in bad] == [engine.SG_EINVAL] * 5
