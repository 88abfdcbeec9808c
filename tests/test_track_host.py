"""K13, the tracks, on the CPU: the pure-Python reference tests/track_ref.py against a second formulation written apart from it (sets
of refs per track and a sort instead of the min / claim arithmetic) over random sequences of windows, hand-written known answers for
every rule of the contract, invariants over the oracle's churn windows, and the plan in alaz_amd/csrc/sg_plan.hpp
(tests/micro/plan_driver.cpp, stage track)."""
import ctypes as C
import os

import numpy as np
import pytest

from alaz_amd import engine, weights
from tests.helpers import CLOCK
from tests.host_scaffold import LABEL, MERGED, NEW, OBIP, SPLIT, _coverage, chain, random_sequence, window_of
from tests.incident_ref import incident_ref, quantile_threshold
from tests.nodes_ref import nodes_ref
from tests.plan_driver import plan_fixture
from tests.plan_layout import check_layout
from tests.traces import churn  # noqa: F401  (the fixture: events only, no engine)
from tests.track_ref import TrackRef, is_anchor

HERE = os.path.dirname(os.path.abspath(__file__))
NO = engine.NO_TRACK


def by_ref(win, rows):
    """{ref: its incident's TRACK_DTYPE row} for the nodes in an incident"""
    nodes, node_inc, _ = win
    return {int(nodes["ref"][v]): rows[int(node_inc[v])] for v in range(len(nodes)) if node_inc[v] != engine.NO_INCIDENT}


# ---- the contract again, on its own: every track owns a set of refs --------------------------------------------------------------------
class TrackSets:
    def __init__(self, quiet, cap):
        self.quiet, self.cap, self.w, self.issued, self.cut = quiet, cap, 0, 0, 0
        self.tracks = []                                              # dict(id, parent, first, last, windows, peak, count, err, refs {ref: window})

    def step(self, nodes, node_inc, incidents):
        w = self.w
        owner = {}                                                    # ref -> the track that holds it and saw it recently enough
        for t in self.tracks:
            for ref, seen in t["refs"].items():
                if w - seen <= self.quiet + 1:
                    owner[ref] = t["id"]
        groups = [[] for _ in incidents]
        for v, i in enumerate(node_inc):
            if i != engine.NO_INCIDENT and (int(nodes["ref"][v]) >> 30) < 2:
                groups[int(i)].append(int(nodes["ref"][v]))
        facts = []
        for i, refs in enumerate(groups):
            touched = sorted({owner[r] for r in refs if r in owner})
            oldest = touched[0] if touched else None
            facts.append(dict(i=i, oldest=oldest, kept=sum(1 for r in refs if owner.get(r) == oldest and oldest is not None),
                              moved=sum(1 for r in refs if r in owner and owner[r] != oldest), joined=sum(1 for r in refs if r not in owner)))
        winner = {}                                                   # track id -> the incident that carries it on
        for t in self.tracks:
            rivals = sorted((f for f in facts if f["oldest"] == t["id"]), key=lambda f: (-f["kept"], f["i"]))
            if rivals:
                winner[t["id"]] = rivals[0]["i"]
        fresh = [f for f in facts if f["oldest"] is None or winner[f["oldest"]] != f["i"]]
        rows = np.zeros(len(incidents), dtype=engine.TRACK_DTYPE)
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


@pytest.mark.parametrize("quiet", [0, 1, 3])
def test_reference_against_the_sets_formulation(quiet):
    met = set()
    for seed in range(12):
        ref, sets = TrackRef(quiet, 0, ncap=64), TrackSets(quiet, (quiet + 1) * 64)
        for w, edges in enumerate(random_sequence(seed)):
            win = window_of(edges)
            before = ref.entries()
            rows, ended = ref.step(*win)
            rows2, ended2 = sets.step(*win)
            assert rows.tobytes() == rows2.tobytes(), (seed, w)
            assert ended.tobytes() == ended2.tobytes(), (seed, w)
            assert ref.entries().tobytes() == sets.entries().tobytes(), (seed, w)
            met |= _coverage(before, rows, ended, ref.entries(), w, quiet)
        assert ref.stats() == dict(windows=30, live=len(sets.tracks), opened=sets.issued, dropped_cap=0)
    want = {"merged", "split_kept", "split_tie", "ended", "expiry"} | ({"revival"} if quiet else set())
    assert want <= met, want - met


def test_a_small_table_cuts_in_the_random_sequences():
    cuts = 0
    for seed in range(12):
        ref, sets = TrackRef(1, 3), TrackSets(1, 3)
        for w, edges in enumerate(random_sequence(seed)):
            win = window_of(edges)
            rows, ended = ref.step(*win)
            rows2, ended2 = sets.step(*win)
            assert rows.tobytes() == rows2.tobytes() and ended.tobytes() == ended2.tobytes(), (seed, w)
            assert ref.entries().tobytes() == sets.entries().tobytes() and len(ref.entries()) <= 3
            assert len(set(rows["track"].tolist())) == len(rows)
        assert ref.stats()["dropped_cap"] == sets.cut
        cuts += sets.cut
    assert cuts > 0


# ---- known answers, one rule each -------------------------------------------------------------------------------------------------------
def test_an_incident_that_stays_keeps_its_track():
    ref = TrackRef(2, 0, ncap=16)
    for w in range(3):
        win = window_of(chain(1, 2, 3))
        rows, ended = ref.step(*win)
        assert len(rows) == 1 and len(ended) == 0
        r = rows[0]
        assert (r["track"], r["parent"], r["first_window"], r["windows"]) == (0, NO, 0, w + 1)
        assert (r["kept_nodes"], r["moved_nodes"], r["joined_nodes"], r["flags"]) == ((0, 0, 3, NEW) if w == 0 else (3, 0, 0, 0))
    e = ref.entries()
    inc = win[2][0]
    assert len(e) == 1 and (e[0]["track"], e[0]["first_window"], e[0]["last_window"], e[0]["windows"], e[0]["peak_nodes"]) == (0, 0, 2, 3, 3)
    assert e[0]["count"] == 3 * int(inc["count"]) and e[0]["err"] == 3 * int(inc["err"])
    assert ref.stats() == dict(windows=3, live=1, opened=1, dropped_cap=0)


def test_a_merge_continues_as_the_older_track_and_ends_the_younger():
    ref = TrackRef(2, 0, ncap=16)
    rows, _ = ref.step(*window_of(chain(1, 2) + chain(5, 6)))
    assert rows["track"].tolist() == [0, 1] and rows["flags"].tolist() == [NEW, NEW]
    young = ref.entries()[1]
    rows, ended = ref.step(*window_of(chain(1, 2, 5, 6, 7)))
    assert len(rows) == 1
    r = rows[0]
    assert (r["track"], r["windows"], r["kept_nodes"], r["moved_nodes"], r["joined_nodes"], r["flags"]) == (0, 2, 2, 2, 1, MERGED)
    assert len(ended) == 1 and ended.tobytes() == young.tobytes() and ended[0]["track"] == 1   # as it stood
    assert ref.entries()["track"].tolist() == [0, 1]                   # the absorbed track stays in the table through its quiet span
    rows, ended = ref.step(*window_of(chain(1, 2, 5, 6, 7)))
    assert (rows[0]["track"], rows[0]["kept_nodes"], rows[0]["moved_nodes"], rows[0]["flags"]) == (0, 5, 0, 0) and len(ended) == 0


@pytest.mark.parametrize("cut,first,second", [(4, (1, 0, 4, NEW | SPLIT), (0, NO, 6, 0)), (5, (0, NO, 5, 0), (1, 0, 5, NEW | SPLIT))])
def test_a_split_continues_in_the_piece_that_kept_most(cut, first, second):
    """pods 1..10 cut into 1..cut and cut+1..10: 4 / 6 goes to the larger piece although it is the later incident, 5 / 5 to the first"""
    ref = TrackRef(2, 0, ncap=16)
    ref.step(*window_of(chain(*range(1, 11))))
    rows, ended = ref.step(*window_of(chain(*range(1, cut + 1)) + chain(*range(cut + 1, 11))))
    assert len(rows) == 2 and len(ended) == 0
    for r, (track, parent, kept, flags) in zip(rows, (first, second)):
        assert (r["track"], r["parent"], r["kept_nodes"], r["moved_nodes"], r["joined_nodes"], r["flags"]) == (track, parent, kept, 0, 0, flags)
    assert rows["first_window"].tolist() == ([1, 0] if cut == 4 else [0, 1])
    e = ref.entries()
    assert e["track"].tolist() == [0, 1] and e["parent"].tolist() == [NO, 0] and e["peak_nodes"].tolist() == [10, cut]


@pytest.mark.parametrize("quiet", [0, 1, 2])
def test_a_flap_keeps_its_id_inside_the_quiet_span_and_expires_after_it(quiet):
    ref = TrackRef(quiet, 0, ncap=16)
    ref.step(*window_of(chain(1, 2, 3)))
    listed = 0
    for _ in range(quiet):
        rows, ended = ref.step(*window_of([]))
        listed += len(ended)
        assert len(rows) == 0 and ref.entries()["track"].tolist() == [0]
    rows, ended = ref.step(*window_of(chain(1, 2, 3)))
    listed += len(ended)
    assert (rows[0]["track"], rows[0]["windows"], rows[0]["kept_nodes"], rows[0]["flags"]) == (0, 2, 3, 0)
    assert listed == (1 if quiet else 0)                              # ended once, in its first silent window
    for k in range(quiet + 1):                                        # one silent window more than it survives
        rows, ended = ref.step(*window_of([]))
        assert len(ended) == (1 if k == 0 else 0)
        assert ref.entries()["track"].tolist() == ([0] if k < quiet else [])
    rows, ended = ref.step(*window_of(chain(1, 2, 3)))
    assert (rows[0]["track"], rows[0]["parent"], rows[0]["windows"], rows[0]["joined_nodes"], rows[0]["flags"]) == (1, NO, 1, 3, NEW)
    assert ref.entries()["track"].tolist() == [1] and len(ended) == 0


def test_an_outbound_ip_never_anchors():
    ref = TrackRef(2, 0, ncap=16)
    win = window_of([(1, OBIP | 0)])
    rows, _ = ref.step(*win)
    assert win[2]["nodes"][0] == 2 and (rows[0]["track"], rows[0]["joined_nodes"], rows[0]["kept_nodes"]) == (0, 1, 0)
    rows, _ = ref.step(*window_of([(2, OBIP | 0)]))                   # the same index is another address now
    assert (rows[0]["track"], rows[0]["parent"], rows[0]["joined_nodes"], rows[0]["kept_nodes"], rows[0]["flags"]) == (1, NO, 1, 0, NEW)
    rows, _ = ref.step(*window_of([(1, OBIP | 5)]))                   # the pod carries its track to whatever address it calls
    assert (rows[0]["track"], rows[0]["kept_nodes"], rows[0]["flags"]) == (0, 1, 0)
    rows, _ = ref.step(*window_of([(3, LABEL | 4)]))
    rows, _ = ref.step(*window_of([(4, LABEL | 4)]))                  # a label is an anchor
    assert (rows[0]["track"], rows[0]["kept_nodes"], rows[0]["joined_nodes"], rows[0]["flags"]) == (2, 1, 1, 0)
    assert is_anchor(LABEL | 4) and is_anchor(7) and not is_anchor(OBIP | 0)


def test_the_table_is_cut_at_max_tracks():
    ref = TrackRef(2, 2)
    pairs = chain(1, 2) + chain(3, 4) + chain(5, 6) + chain(7, 8)
    rows, _ = ref.step(*window_of(pairs))
    assert rows["track"].tolist() == [0, 1, 2, 3] and ref.entries()["track"].tolist() == [0, 1]
    assert ref.stats() == dict(windows=1, live=2, opened=4, dropped_cap=2)
    rows, ended = ref.step(*window_of(pairs))                          # a member that names an id the table lacks is not live
    assert rows["track"].tolist() == [0, 1, 4, 5] and rows["flags"].tolist() == [0, 0, NEW, NEW] and rows["parent"].tolist() == [NO] * 4
    assert rows["joined_nodes"].tolist() == [0, 0, 2, 2] and len(ended) == 0
    assert ref.entries()["track"].tolist() == [0, 1] and ref.stats() == dict(windows=2, live=2, opened=6, dropped_cap=4)


def test_dtype_and_struct_sizes():
    assert engine.TRACK_DTYPE.itemsize == 32 and engine.TRACK_ENTRY_DTYPE.itemsize == 40 and C.sizeof(engine.SgTrackParams) == 16
    d = engine.TRACK_ENTRY_DTYPE
    assert [d.fields[f][1] for f in ("track", "last_window", "peak_nodes", "count", "err")] == [0, 12, 20, 24, 32]
    assert engine.TRACK_DTYPE.names == ("track", "parent", "first_window", "windows", "kept_nodes", "moved_nodes", "joined_nodes", "flags")
    assert C.sizeof(engine.SgTrackStats) == 32 and NO == 0xFFFFFFFF and (NEW, SPLIT, MERGED) == (1, 2, 4)


# ---- the oracle's churn windows at a fixed threshold ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_windows(churn, oracle_lib):  # noqa: F811
    topo, labels, wins = churn
    o = oracle_lib.Oracle(*CLOCK); o.apply_ops(topo.k8s_ops())
    W = weights.make_weights(2)
    out = []
    for w in wins:
        o.packed(w, labels); o.window_close(W, 2)
        rows = o.edge_rows()
        out.append((rows, nodes_ref(rows)))
    return out


@pytest.mark.parametrize("quiet", [0, 2])
def test_invariants_over_the_oracle_windows(oracle_windows, quiet):
    thr = quantile_threshold(oracle_windows[0][0]["score"], 0.9)
    ncap = max(len(n) for _, n in oracle_windows)
    ref, sets = TrackRef(quiet, 0, ncap=ncap), TrackSets(quiet, (quiet + 1) * ncap)
    seen, continued = set(), 0
    for w, (rows, nodes) in enumerate(oracle_windows):
        inc, node_inc = incident_ref(rows, nodes, "score", thr)
        assert len(inc) > 0
        tr, ended = ref.step(nodes, node_inc, inc)
        tr2, ended2 = sets.step(nodes, node_inc, inc)
        assert tr.tobytes() == tr2.tobytes() and ended.tobytes() == ended2.tobytes() and ref.entries().tobytes() == sets.entries().tobytes()
        anchors = np.zeros(len(inc), np.int64)
        for v, i in enumerate(node_inc):
            if i != engine.NO_INCIDENT and is_anchor(nodes["ref"][v]):
                anchors[i] += 1
        assert (tr["kept_nodes"].astype(np.int64) + tr["moved_nodes"] + tr["joined_nodes"] == anchors).all() and (anchors > 0).all()
        assert len(set(tr["track"].tolist())) == len(tr)               # ids unique within a window
        assert (tr["windows"].astype(np.int64) <= w - tr["first_window"].astype(np.int64) + 1).all()
        fresh = tr["track"][(tr["flags"] & NEW) != 0].tolist()
        assert not set(fresh) & seen and fresh == sorted(fresh)       # an id is never reused
        seen |= set(tr["track"].tolist())
        continued += int(((tr["flags"] & NEW) == 0).sum())
        e = ref.entries()
        assert (np.diff(e["track"].astype(np.int64)) > 0).all() and (w - e["last_window"].astype(np.int64) <= quiet).all()
        assert set(ended["track"].tolist()) <= set(e["track"].tolist()) if quiet else not set(ended["track"].tolist()) & set(e["track"].tolist())
    assert continued > 0 and ref.stats()["opened"] == len(seen)


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------
track_plan = plan_fixture("track")


def _p(mk, ml, nc, slots=1, ss=16, quiet=2, mt=0, res=0):
    return (mk, ml, nc, slots, ss, quiet, mt, res)


# (max_known, max_labels, ncap): toy, config 3, a 400 k-node shard of config 5
ENGINES = [(1024, 16, 1100), (12_000, 1000, 15_000), (380_000, 4000, 400_000), (1, 0, 1), (0, 0, 0)]


def test_plan_sizes(track_plan):
    for r in track_plan([_p(mk, ml, nc, slots, quiet=q, mt=mt) for mk, ml, nc in ENGINES for slots in (1, 3) for q in (0, 2, 15) for mt in (0, 8, 100_000)]):
        assert r["rc"] == 0 and (r["row_size"], r["entry_size"], r["params_size"], r["stats_size"]) == (32, 40, 16, 32)
        nc, slots = max(r["ncap"], 1), r["slots"]
        mt = r["max_tracks"]
        assert mt in (8, 100_000) or mt == (r["quiet"] + 1) * nc
        span = max(nc, mt)
        assert r["threads"] == 256 and r["per"] % 256 == 0 and 1 <= r["wgs"] <= r["max_wgs"] == 1024
        assert r["wgs"] * r["per"] >= span > (r["wgs"] - 1) * r["per"]
        assert 1 <= r["init_wgs"] <= 1024 and 1 <= r["node_wgs"] <= 1024 and r["node_wgs"] == min(1024, -(-nc // 256))
        assert r["fold_rounds"] == 8 and r["fold_wgs"] == min(1024, -(-nc // 2048))   # a workgroup of the folding passes: 2048 node rows
        assert r["anchors"] == r["max_known"] + r["max_labels"] and r["member_bytes"] >= 4 * r["anchors"]
        assert r["table_bytes"] >= 40 * mt and r["claim_bytes"] >= 8 * mt and r["inc_bytes"] >= 4 * nc and r["state_bytes"] >= 24
        assert r["blk_bytes"] >= 7 * 1024 * 4 and r["rows_bytes"] >= 32 * nc and r["ended_bytes"] >= 40 * nc and r["count_bytes"] >= 8
        for k in ("member_bytes", "table_bytes", "state_bytes", "inc_bytes", "claim_bytes", "blk_bytes", "rows_bytes", "ended_bytes", "count_bytes"):
            assert r[k] % 256 == 0
        assert r["total_bytes"] == (2 * r["member_bytes"] + 2 * r["table_bytes"] + 2 * r["state_bytes"] + 6 * r["inc_bytes"] + r["claim_bytes"]
                                    + r["blk_bytes"] + slots * (r["rows_bytes"] + r["ended_bytes"] + r["count_bytes"]))
        check_layout(r, {"mtrack": 4 * r["anchors"], "mlast": 4 * r["anchors"], "table0": 40 * mt, "table1": 40 * mt, "state0": 24, "state1": 24,
                         **{k: 4 * nc for k in ("cand", "kept", "moved", "joined", "pos", "tv")}, "claim": 8 * mt, "blk": 7 * 1024 * 4,
                         "rows": 32 * nc, "ended": 40 * nc, "ended_count": 8}, per_slot=("rows", "ended", "ended_count"))
        # 8 B an anchor, 88 B a table position, (24 + 72 x slots) B a node key, the counts, 256 B of rounding a piece
        assert r["total_bytes"] <= 8 * r["anchors"] + 88 * mt + (24 + 72 * slots) * nc + 7 * 4096 + 256 * (14 + 3 * slots)
    c3, = track_plan([_p(12_000, 1000, 15_000)])
    assert (c3["max_tracks"], c3["wgs"], c3["per"], c3["node_wgs"], c3["fold_wgs"]) == (45_000, 176, 256, 59, 8) and c3["total_bytes"] < 6 << 20
    toy, = track_plan([_p(1408, 16, 1492)])                           # tests/test_gpu_tracks.py's 1 400-pod engine: one folding workgroup
    assert toy["fold_wgs"] == 1 and toy["node_wgs"] == 6
    big, = track_plan([_p(380_000, 4000, 400_000)])
    assert (big["max_tracks"], big["wgs"], big["per"]) == (1_200_000, 938, 1280) and big["total_bytes"] < 160 << 20


def test_plan_parameter_checks(track_plan):
    ok = track_plan([_p(1000, 10, 100, quiet=q) for q in (0, 1, 15)])
    assert [r["rc"] for r in ok] == [0] * 3 and [r["max_tracks"] for r in ok] == [100, 200, 1600]
    assert track_plan([_p(1000, 10, 100, mt=7)])[0]["max_tracks"] == 7
    bad = track_plan([_p(1000, 10, 100, quiet=16), _p(1000, 10, 100, ss=12), _p(1000, 10, 100, ss=20), _p(1000, 10, 100, res=1),
                      _p(1000, 10, 1 << 28, quiet=15)])
    assert [r["rc"] for r in bad] == [engine.SG_EINVAL] * 5
