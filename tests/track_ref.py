"""Pure-Python reference of the tracks (K13, include/servicegraph.h "tracks").

TrackRef(quiet_windows, max_tracks, ncap) keeps the contract's state in Python ints, keyed by ref: the members {ref: (track, last)}
and the track table, a list of dicts ascending by id.  step(nodes, node_inc, incidents) takes one window's node rows, the incident
per node row and the incident rows (numpy structured arrays as the engine returns them) and returns (TRACK_DTYPE rows, the ended
TRACK_ENTRY_DTYPE entries).  entries() is the live table, stats() the counters.  Every field is an integer sum, an integer max, a
min of ids or the max of a (kept << 32 | ~incident) key: the device result must equal it byte for byte."""
import numpy as np

from alaz_amd.engine import NO_INCIDENT, NO_TRACK, TRACK_DTYPE, TRACK_ENTRY_DTYPE, TRACK_MERGED, TRACK_NEW, TRACK_SPLIT

U64 = (1 << 64) - 1
U32 = (1 << 32) - 1
ENTRY_FIELDS = ("track", "parent", "first_window", "last_window", "windows", "peak_nodes", "count", "err")


def is_anchor(ref):
    """a KNOWN or LABEL ref (SG_REF_TYPE 0 or 1); an OBIP ref is an index into one window's outbound-IP list"""
    return (int(ref) >> 30) in (0, 1)


def entries_array(entries):
    out = np.zeros(len(entries), dtype=TRACK_ENTRY_DTYPE)
    for k, e in enumerate(entries):
        for f in ENTRY_FIELDS:
            out[k][f] = e[f]
    return out


class TrackRef:
    def __init__(self, quiet_windows=2, max_tracks=0, ncap=None):
        assert 0 <= quiet_windows <= 15
        if not max_tracks:
            assert ncap is not None, "max_tracks = 0 means (quiet_windows + 1) * ncap"
            max_tracks = (quiet_windows + 1) * max(ncap, 1)
        self.q, self.max_tracks = quiet_windows, max_tracks
        self.w = 0
        self.next_id = 0
        self.member = {}                                              # ref -> (track, last)
        self.table = []                                               # dicts, ascending by id
        self.dropped_cap = 0

    def _tv(self, ref, held):
        m = self.member.get(ref)
        if m is None:
            return NO_TRACK
        T, l = m
        return T if self.w - l - 1 <= self.q and T in held else NO_TRACK

    def step(self, nodes, node_inc, incidents):
        w, q = self.w, self.q
        I = len(incidents)
        held = {e["track"]: p for p, e in enumerate(self.table)}      # (every stored entry is live at w: step 9 of w - 1 kept only those)
        for e in self.table:
            assert w - e["last_window"] - 1 <= q
        anchors = [[] for _ in range(I)]                              # (ref, t_v) of every anchor, per incident
        for v in range(len(nodes)):
            i = int(node_inc[v])
            if i == NO_INCIDENT:
                continue
            ref = int(nodes["ref"][v])
            if is_anchor(ref):
                anchors[i].append((ref, self._tv(ref, held)))
        cand, kept, moved, joined = [], [], [], []
        for i in range(I):
            assert anchors[i], "every incident has an anchor: every row has a pod at one end"
            c = min(t for _, t in anchors[i])                         # (SG_NO_TRACK is the largest u32)
            cand.append(c)
            kept.append(sum(1 for _, t in anchors[i] if t == c != NO_TRACK))
            moved.append(sum(1 for _, t in anchors[i] if t != NO_TRACK and t != c))
            joined.append(sum(1 for _, t in anchors[i] if t == NO_TRACK))
        claim = {}                                                    # track -> (kept << 32 | ~i) max
        for i in range(I):
            if cand[i] != NO_TRACK:
                key = (kept[i] << 32) | (~i & U32)
                claim[cand[i]] = max(claim.get(cand[i], 0), key)
        rows = np.zeros(I, dtype=TRACK_DTYPE)
        opened, cont_of = [], {}
        for i in range(I):
            c = cand[i]
            r = rows[i]
            r["kept_nodes"], r["moved_nodes"], r["joined_nodes"] = kept[i], moved[i], joined[i]
            flags = TRACK_MERGED if moved[i] else 0
            if c != NO_TRACK and (~claim[c] & U32) == i:
                e = self.table[held[c]]
                cont_of[c] = i
                r["track"], r["parent"], r["first_window"], r["windows"] = c, e["parent"], e["first_window"], e["windows"] + 1
            else:
                T = self.next_id + len(opened)
                flags |= TRACK_NEW | (TRACK_SPLIT if c != NO_TRACK else 0)
                r["track"], r["parent"], r["first_window"], r["windows"] = T, c, w, 1
                opened.append(dict(track=T, parent=c, first_window=w, last_window=w, windows=1, peak_nodes=int(incidents["nodes"][i]),
                                   count=int(incidents["count"][i]), err=int(incidents["err"][i])))
            r["flags"] = flags
        self.next_id += len(opened)
        ended = [dict(e) for e in self.table if e["track"] not in cont_of and e["last_window"] == w - 1]
        new = []
        for e in self.table:
            if e["track"] in cont_of:
                i = cont_of[e["track"]]
                e = dict(e, last_window=w, windows=e["windows"] + 1, peak_nodes=max(e["peak_nodes"], int(incidents["nodes"][i])),
                         count=(e["count"] + int(incidents["count"][i])) & U64, err=(e["err"] + int(incidents["err"][i])) & U64)
                new.append(e)
            elif w - e["last_window"] <= q:
                new.append(e)
        new += opened
        self.dropped_cap += max(0, len(new) - self.max_tracks)
        self.table = new[: self.max_tracks]
        for i in range(I):
            for ref, _ in anchors[i]:
                self.member[ref] = (int(rows["track"][i]), w)
        self.w += 1
        return rows, entries_array(ended)

    def entries(self):
        return entries_array(self.table)

    def stats(self):
        return dict(windows=self.w, live=len(self.table), opened=self.next_id, dropped_cap=self.dropped_cap)
