"""The K6 halo kernels (alaz_amd/csrc/sg_k6.h) against tests/halo_ref.py, list for list, and their pack / unpack kernels as copies.

Every other sharded test judges K6 through the scored rows, and rows cannot see a request list that is a superset of the right one,
a capacity overflow (no other test makes one) or any builder but the default one.  Here every list builder runs:

  form             engine                                     kernel
  lists            shipped library                            k6_halo_lists                      (many workgroups, look-back)
  one_wg           development build, SG_K6_ONE_WG=1          k6_halo_build_padded<true>         (staged, wave-ordered)
  one_wg_big       ... and a node capacity > 49 152           k6_halo_build_padded<false>        (N <= 49 152: falls back to the staged form;
                                                                                                  N > 49 152: the general form, DPP scans)
  unpadded         shipped library, sg_halo_build             k6_active_lists<true> + k6_halo_build, k6_pack / k6_unpack
  unpadded_big     node capacity > 49 152, sg_halo_build      k6_active_lists<false> + k6_halo_build

and the lists they write are compared with the reference word for word: the count, the ids, and the sentinel the test wrote
beforehand in every word behind a list and behind the buffer.  The active lists (act_l, act_p) are not exposed; they are held through
the rows: the layer buffers are the test's own tensors, filled with NaN before every window, so a node missing from act_l shows in
a score, and the concatenated rows must be the unsharded engine's byte for byte — for every form.

All shard engines live on one device and one stream and are driven one after the other from one thread; the gather of the outbound
IPs, the two statistics all-reduces and the all-to-alls are torch copies between the shards' buffers.  (sg_window_run is the only
call that rotates an engine's window slots; neither this staged sequence nor sg_window_run_sharded does: a sharded engine has ONE
working slot however many it was created with, so there is no "two windows in flight" variant here.)

That SG_K6_ONE_WG=1 reaches the plan (plan.k6_one_wg) is held on the CPU by tests/test_plan.py; launch_halo_lists branches on that
field alone."""
import os

import numpy as np
import pytest

from alaz_amd import replay, sharded, weights
from tests import halo_ref
from tests.helpers import CLOCK

pytestmark = pytest.mark.gpu

SENT = -1515870811                  # 0xA5A5A5A5 as the int32 the list buffers hold: no node id, no count
GUARD = 64                          # sentinel words behind every buffer
FLAGS_LDS = 49_152                  # K6_FLAGS_LDS of sg_k6.h
KNOB = "SG_K6_ONE_WG"
WORLDS = (2, 3, 8)

#: form -> (development build with SG_K6_ONE_WG=1, node capacity beyond K6_FLAGS_LDS, the unpadded API)
FORMS = {"lists": (False, False, False), "one_wg": (True, False, False), "one_wg_big": (True, True, False),
         "unpadded": (False, False, True), "unpadded_big": (False, True, True)}


def _key(a):
    return np.lexsort((a["to_ref"], a["from_ref"]))


def _register(g, topo):
    """pods 0 .. P-1, services P .. P+S-1: the ids HostShim gives topo.k8s_ops()"""
    for i, ip in enumerate(topo.pod_ips.tolist()):
        g.upsert_pod(ip, i)
    for j, ip in enumerate(topo.svc_ips.tolist()):
        g.upsert_service(ip, topo.n_pods + j)


def _feed(g, ev):
    for i in range(0, len(ev), 1 << 15):
        while g.ingest(ev[i:i + (1 << 15)]) != 0:
            pass


class Case:
    """a map and what the unsharded engine makes of each of its windows: rows, outbound IPs, node counts (made once per module)"""
    def __init__(self, topo, windows, n_labels, layers=2, max_labels=3072, max_obip=512, engine_kw=None):
        self.topo, self.windows, self.n_labels, self.layers = topo, windows, n_labels, layers
        self.max_labels, self.max_obip, self.engine_kw = max_labels, max_obip, engine_kw or {}
        self.pod = {int(ip): i for i, ip in enumerate(topo.pod_ips)}
        self.svc = {int(ip): topo.n_pods + j for j, ip in enumerate(topo.svc_ips)}
        self.want = []
        g = self.engine(0, 1, False, False)
        try:
            g.set_label_count(n_labels)
            for ev in windows:
                if len(ev): _feed(g, ev)
                rows = g.flush_window().copy()
                st = g.stats()
                self.want.append((rows[_key(rows)], g.outbound_ips().copy(), int(st.last_window_nodes)))
            assert st.events_dropped_cap == 0
        finally:
            g.close()

    def engine(self, rank, world, one_wg, big):
        from alaz_amd import engine
        os.environ.pop(KNOB, None)
        if one_wg: os.environ[KNOB] = "1"
        try:
            g = engine.ServiceGraph(max_known_nodes=self.topo.n_nodes, max_edges=16384, layers=self.layers,
                                    max_labels=FLAGS_LDS + 1024 if big else self.max_labels, max_outbound_ips=self.max_obip, rank=rank, world=world,
                                    max_batch=1 << 15, max_window_events=1 << 16, dev_knobs=one_wg, **self.engine_kw)
        finally:
            os.environ.pop(KNOB, None)
        g.set_clock(*CLOCK); g.load_weights(weights.make_weights(self.layers)); _register(g, self.topo)
        return g

    def ncap(self, big):
        return self.topo.n_nodes + (FLAGS_LDS + 1024 if big else self.max_labels) + self.max_obip

    def ref(self, w, world, pad=0):
        """the reference of window w with `pad` label nodes beyond the trace's own"""
        rows, ob, n = self.want[w]
        r = halo_ref.HaloRef(rows["from_ref"], rows["to_ref"], ob, self.topo.n_nodes, self.n_labels + pad, world)
        assert r.N == n + pad                                            # the unsharded engine's own node count
        return r


_CASES = {}


def _case(name):
    if name not in _CASES:
        if name in halo_ref.TOPO_CASES:
            topo, ev, labels = halo_ref.topo_trace(*halo_ref.TOPO_CASES[name])
            c = Case(topo, [ev], len(labels))
        elif name == "small":
            topo, ev, labels = halo_ref.small_trace()
            c = Case(topo, [ev], 0)
        elif name == "empty":                                            # the tables of t120, a window without events
            topo, ev, labels = halo_ref.topo_trace(*halo_ref.TOPO_CASES["t120"])
            c = Case(topo, [ev[:0]], len(labels))
        elif name == "one":                                              # one pod that talks to itself: N = 1
            topo, ev, labels = halo_ref.one_trace()
            c = Case(topo, [ev], 0)
        elif name in ("shrink", "shrink_warm"):
            topo, wins, labels = halo_ref.shrink_windows()
            if name == "shrink_warm": c = Case(topo, [wins[0], wins[1], wins[0]], len(labels), max_obip=4096, engine_kw=dict(k1_variant=3, warm=True))
            else: c = Case(topo, wins, len(labels), max_obip=4096)
        elif name == "large":
            topo, ev, labels = halo_ref.large_map_trace()
            c = Case(topo, [ev], len(labels), layers=1, max_labels=128)
        _CASES[name] = c
    return _CASES[name]


class Shards:
    """`world` shard engines of a case on device 0, all on one stream, and the sharded window driven over them rank by rank"""
    def __init__(self, case, world, form, halo_cap=0):
        import torch
        self.torch, self.case, self.world, self.form = torch, case, world, form
        self.one_wg, self.big, self.unpadded = FORMS[form]
        self.dev = torch.device("cuda", 0)
        self.engs = []
        try:
            for r in range(world):
                self.engs.append(case.engine(r, world, self.one_wg, self.big))
            self.stream = torch.cuda.Stream(self.dev)
            # (a node capacity beyond 49 152 would make the default per-pair capacity tens of thousands of rows: 4096 holds every list here)
            cap = halo_cap or (4096 if self.big else 0)
            with torch.cuda.stream(self.stream):
                self.bes = [sharded.HipBackend(g, ncap=case.ncap(self.big), layers=case.layers, world=world, rank=r, device=self.dev,
                                               max_obip=case.max_obip, stream=self.stream, halo_cap=cap) for r, g in enumerate(self.engs)]
                self.capp = self.bes[0].capp
                for be in self.bes:                                      # the request lists with sentinel words behind the last row
                    be.req_all = torch.full((world * (self.capp + 1) + GUARD,), SENT, dtype=torch.int32, device=self.dev)
                    be.req = be.req_all[: world * (self.capp + 1)].view(world, self.capp + 1)
            self.stream.synchronize()
        except Exception:
            self.close()
            raise

    def close(self):
        for g in self.engs: g.close()
        self.engs = []

    def __enter__(self): return self
    def __exit__(self, *a): self.close()

    def set_form(self, form):
        assert FORMS[form][:2] == (self.one_wg, self.big)
        self.form, self.unpadded = form, FORMS[form][2]

    def overflow(self):
        return [int(g.stats().halo_overflow) for g in self.engs]

    def window(self, ev, n_labels, unpadded_cap=None):
        """one window over all shards.  Returns per rank the request buffer as it stood behind the builder (padded forms: the whole
        [world][capp + 1] buffer and its guard words; unpadded: (counts, ids with guard)), the concatenated rows in canonical order,
        and the shards' node counts.  unpadded_cap: room of the unpadded call's id buffer (default: more than any list needs)."""
        torch, world, bes, engs = self.torch, self.world, self.bes, self.engs
        shard = sharded.route_events(ev, world, self.case.pod, self.case.svc) if len(ev) else np.zeros(0, np.uint32)
        for r, g in enumerate(engs):
            part = ev[shard == r]
            if len(part): _feed(g, part)
            g.set_label_count(n_labels)
        lists = []
        with torch.cuda.stream(self.stream):
            for be in bes:
                for f in be.feat: f.fill_(float("nan"))                  # a layer row nobody writes shows in a score
            ob = torch.stack([be.ob_local().clone() for be in bes])
            for be in bes:
                be.ob_all.copy_(ob); be.close_gathered()
            s = torch.stack([be.stats_sum for be in bes]).sum(dim=0); m = torch.stack([be.stats_max for be in bes]).max(dim=0).values
            for be in bes:
                be.stats_sum.copy_(s); be.stats_max.copy_(m); be.features()
            if self.unpadded:
                cap = 4096 if unpadded_cap is None else unpadded_cap
                ids = [torch.full((cap + GUARD,), SENT, dtype=torch.int32, device=self.dev) for _ in bes]
                cnt = [torch.full((8 + GUARD,), SENT, dtype=torch.int32, device=self.dev) for _ in bes]
                for r, g in enumerate(engs):
                    g.halo_build(ids[r].data_ptr(), cap, cnt[r].data_ptr(), bes[r].s)
                self.stream.synchronize()
                lists = [(cnt[r].cpu().numpy(), ids[r].cpu().numpy()) for r in range(world)]
                n = [[int(x) for x in lists[r][0][:world]] for r in range(world)]
                self._usable([c for r in range(world) for c in n[r]] + [sum(n[r]) for r in range(world)], cap,
                             [lists[r][1][: max(0, min(cap, sum(n[r])))] for r in range(world)])
                off = [np.concatenate([[0], np.cumsum(n[r])]) for r in range(world)]
                for l in range(1, self.case.layers + 1):
                    for be in bes: be.layer(l - 1)
                    for r in range(world):                               # requester r, owner k: pack on k, copy, unpack on r
                        for k in range(world):
                            if n[r][k] == 0: continue
                            p = ids[r].data_ptr() + 4 * int(off[r][k])
                            out = torch.zeros(n[r][k], 64, dtype=torch.float32, device=self.dev)
                            engs[k].halo_pack(l, p, n[r][k], out.data_ptr(), bes[k].s)
                            got = out.clone()
                            engs[r].halo_unpack(l, p, n[r][k], got.data_ptr(), bes[r].s)
            else:
                for be in bes:
                    be.req_all.fill_(SENT)
                    be.halo_requests()
                keep = [be.req_all.clone() for be in bes]
                self.stream.synchronize()
                body = [k[: world * (self.capp + 1)].view(world, self.capp + 1).cpu().numpy() for k in keep]
                self._usable([int(c) for x in body for c in x[:, 0]], self.capp,
                             [x[k, 1:1 + max(0, min(self.capp, int(x[k, 0])))] for x in body for k in range(world)])
                for r, be in enumerate(bes):
                    be.serve.copy_(torch.stack([bes[k].req[r] for k in range(world)]))
                for l in range(1, self.case.layers + 1):
                    for be in bes: be.layer(l - 1)
                    outs = [be.pack(l) for be in bes]
                    for r, be in enumerate(bes):
                        be.rows_in.copy_(torch.stack([outs[k][r] for k in range(world)]))
                        be.unpack(l)
                lists = [k.cpu().numpy() for k in keep]
            for be in bes: be.score()
        self.stream.synchronize()
        rows = [g.window_read().copy() for g in engs]
        for g, be in zip(engs, bes): g.window_reset(be.s)
        self.stream.synchronize()
        st = [g.stats() for g in engs]
        assert sum(x.events_dropped_cap + x.events_misrouted for x in st) == 0
        rows = np.concatenate(rows)
        return lists, rows[_key(rows)], [int(x.last_window_nodes) for x in st]

    def _usable(self, counts, cap, ids):
        """before any pack / unpack kernel walks the lists: a count the builder did not write (the sentinel) or one beyond the capacity, or
        an id that is no node, would send those kernels outside the buffers — a wrong builder must fail this test, not fault the device.
        The windows are discarded, the engines stay usable."""
        ok = all(0 <= c <= cap for c in counts) and all(((x >= 0) & (x < self.case.ncap(self.big))).all() for x in ids)
        if not ok:
            for g, be in zip(self.engs, self.bes): g.window_reset(be.s)
            self.stream.synchronize()
        assert ok, (self.form, "a list's count word or ids are not usable", [c for c in counts if not 0 <= c <= cap][:4])

    def check_lists(self, lists, ref, capp=None, unpadded_cap=None):
        """every word of every rank's buffer: counts, ids, sentinels"""
        world = self.world
        for r in range(world):
            if self.unpadded:
                cap = 4096 if unpadded_cap is None else unpadded_cap
                cnt, ids = lists[r]
                want_cnt, want_ids = ref.unpadded(r, cap)
                assert cnt[:world].tolist() == want_cnt, (self.form, r)
                assert (cnt[world:] == SENT).all(), (self.form, r)           # counts[k] is written for k < world only
                assert ids[: len(want_ids)].tolist() == want_ids, (self.form, r)
                assert (ids[len(want_ids):] == SENT).all(), (self.form, r)
            else:
                capp = self.capp
                buf = lists[r]
                want_cnt, want_ids, _ = ref.padded(r, capp)
                assert want_cnt[r] == 0
                body = buf[: world * (capp + 1)].reshape(world, capp + 1)
                for k in range(world):
                    assert int(body[k, 0]) == want_cnt[k], (self.form, r, k, int(body[k, 0]), want_cnt[k])
                    assert body[k, 1:1 + want_cnt[k]].tolist() == want_ids[k], (self.form, r, k)
                    assert (body[k, 1 + want_cnt[k]:] == SENT).all(), (self.form, r, k)
                assert (buf[world * (capp + 1):] == SENT).all(), (self.form, r)


def _padded_bytes(lists, world, capp):
    """the padded lists without their padding: what two forms with different capacities must agree on"""
    out = []
    for buf in lists:
        body = buf[: world * (capp + 1)].reshape(world, capp + 1)
        out.append([body[k, : 1 + max(0, int(body[k, 0]))].tobytes() for k in range(world)])
    return out


def _run_all_forms(case_name, world, pads, forms=tuple(FORMS), precondition=None):
    """every form over the case's windows (one window per entry of `pads` when the case has a single trace: the same events, the
    label count raised to place N); lists against the reference, forms against one another, rows against the unsharded engine"""
    case = _case(case_name)
    seq = [(0, p) for p in pads] if len(case.windows) == 1 else [(w, 0) for w in range(len(case.windows))]
    refs = [case.ref(w, world, pad) for w, pad in seq]
    if precondition: precondition(refs)
    first = {}
    groups = {}
    for form in forms:                                                   # forms that differ in the call only share their engines
        groups.setdefault(FORMS[form][:2], []).append(form)
    for group in groups.values():
        with Shards(case, world, group[0]) as sh:
            for i, (w, pad) in enumerate(seq):
                for form in group:
                    sh.set_form(form)
                    lists, rows, nn = sh.window(case.windows[w], case.n_labels + pad)
                    assert nn == [refs[i].N] * world, (form, i, nn, refs[i].N)   # the case sits on the N it was made for
                    sh.check_lists(lists, refs[i])
                    assert rows.tobytes() == case.want[w][0].tobytes(), (form, i)
                    if not sh.unpadded:
                        b = _padded_bytes(lists, world, sh.capp)
                        assert first.setdefault(i, (form, b))[1] == b, (form, first[i][0], i)
            assert sh.overflow() == [0] * world
    return refs


def _pads(case_name, targets):
    """label pads that put the case's single window on each N of `targets` (ascending: an engine's label count never shrinks)"""
    n0 = _case(case_name).want[0][2]
    assert list(targets) == sorted(targets) and targets[0] >= n0, (n0, targets)
    return [t - n0 for t in targets]


def _nonempty(world):
    def check(refs):
        for ref in refs:
            off = ref.pair_sizes()[~np.eye(world, dtype=bool)]
            assert (off > 0).all() if world < 8 else int((off > 0).sum()) >= 48, off
    return check


@pytest.fixture(scope="module", autouse=True)
def _forget_cases():
    yield
    _CASES.clear()


# ---- a. request lists, every builder, list for list (and d. the active lists, through the rows) ---------------------------------
@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("name", list(halo_ref.TOPO_CASES))
def test_lists_of_every_form_on_a_graph_and_on_workgroup_boundaries(name, world):
    """180 / 1 050 / 3 000 known nodes with enough events to touch the edges: every (shard, owner) list is non-empty at worlds 2 and 3,
    at least 48 of 56 at world 8 (asserted from the reference).  The same events again with the label count raised put a graph whose
    members fill the blocks on k6_halo_lists' workgroup boundaries: N = 1023, 1024, 1025 for the 180-node map, 2048 and 2049 for the
    1 050-node map; the 3 000-node map has four workgroups of members as it is."""
    n0 = _case(name).want[0][2]
    targets = {"t120": [n0, 1023, 1024, 1025], "t700": [n0, 2048, 2049], "t2000": [n0]}[name]
    assert {"t120": n0 < 1023, "t700": 1025 < n0 < 2048, "t2000": 3000 < n0 < 4096}[name], n0
    _run_all_forms(name, world, _pads(name, targets), precondition=_nonempty(world))


@pytest.mark.parametrize("world", WORLDS)
def test_lists_of_every_form_on_small_and_boundary_node_counts(world):
    """62 nodes of a map without Host labels, then N = 63, 64, 65 (one wave and one either side), 1023, 1024, 1025, 2048, 2049 (one and two
    workgroups of k6_halo_lists and one either side) and 3000 by the label count alone: the members are the 60 known nodes at the bottom
    and the two raw outbound IPs, with out-edges of their own, at N - 2 and N - 1 — in the last workgroup, the last wave, the last lane."""
    def some(refs):
        for ref in refs:
            ps = ref.pair_sizes()
            assert ps.sum() > 0 and any(x >= ref.N - 2 for r in range(world) for l in ref.req(r) for x in l), ps
    _run_all_forms("small", world, _pads("small", [63, 64, 65, 1023, 1024, 1025, 2048, 2049, 3000]), precondition=some)


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("name", ["one", "empty"])
def test_lists_of_every_form_on_one_node_and_on_an_empty_window(name, world):
    """N = 1 (one pod talking to itself: one shard has one row, the others none) and a window without events over a registered map:
    every count word 0, nothing else written, rows as the unsharded engine's (one row / none)."""
    refs = _run_all_forms(name, world, [0])
    assert refs[0].N == (1 if name == "one" else 180 + 64) and refs[0].pair_sizes().sum() == 0


@pytest.mark.parametrize("world", WORLDS)
def test_lists_of_the_general_form_on_a_map_beyond_the_lds_staging(world):
    """N = 49 294 > 49 152: with SG_K6_ONE_WG=1 the one-workgroup builder takes its general form (a chunk of 49 nodes per thread, node flags
    from memory, ten DPP scans), k6_halo_lists walks 49 workgroups' totals, and sg_halo_build runs k6_active_lists<false> in the general
    form.  The one case with a large table: a few thousand events over 4 000 edges of 49 200 registered nodes."""
    def some(refs):
        assert refs[0].N > FLAGS_LDS and (refs[0].pair_sizes()[~np.eye(world, dtype=bool)] > 0).sum() >= world * (world - 1) * 3 // 4
    _run_all_forms("large", world, [0], forms=("lists", "one_wg_big", "unpadded_big"), precondition=some)


# ---- b. several windows on one engine -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [3, 8])
def test_lists_over_three_windows_whose_node_count_shrinks_and_grows_again(world):
    """N ~ 2950, ~ 510, ~ 2910 on the same engines (the label count of an engine never shrinks, so the windows differ in their raw
    outbound IPs: 2 700, 250, 2 650): k6_halo_lists runs 3, 1, 3 workgroups, so the middle window leaves the totals of two workgroups
    from an older epoch behind N, and the third must not take them for its own; `cursor` marks and the active lists of the window
    before must be gone.  Every form, every window against the reference."""
    refs = _run_all_forms("shrink", world, [0], precondition=_nonempty(world))
    assert refs[0].N > 2048 and refs[1].N < 1024 and refs[2].N > 2048, [r.N for r in refs]


def test_lists_of_warm_engines_repeat_when_the_trace_repeats():
    """eight warm shard engines (k1_variant 3, kept edge set): window 3 repeats window 1's trace behind a smaller window 2 and closes
    from the kept state — its lists are window 1's byte for byte, and all three equal the reference."""
    world, case = 8, _case("shrink_warm")
    refs = [case.ref(w, world) for w in range(3)]
    kept = []
    with Shards(case, world, "lists") as sh:
        assert all(g.geometry()["warm_windows"] == 1 for g in sh.engs)
        for w in range(3):
            lists, rows, nn = sh.window(case.windows[w], case.n_labels)
            assert nn == [refs[w].N] * world
            sh.check_lists(lists, refs[w])
            assert rows.tobytes() == case.want[w][0].tobytes(), w
            kept.append([l.tobytes() for l in lists])
        assert sh.overflow() == [0] * world
    assert kept[2] == kept[0] and kept[1] != kept[0]


# ---- c. overflow is counted and stays in bounds ---------------------------------------------------------------------------------
def _overflow_capp(ref, world):
    """a capacity from the reference at which some pair overflows and some non-empty pair does not"""
    off = np.sort(ref.pair_sizes()[~np.eye(world, dtype=bool)])
    off = off[off > 0]
    capp = int(off[len(off) // 2])
    if capp == off[-1]: capp = int(off[0])
    assert off[0] <= capp < off[-1], off
    return capp


@pytest.mark.parametrize("form,name,capp", [("lists", "t120", 0), ("lists", "small", 1), ("one_wg", "t120", 0), ("one_wg", "small", 1),
                                            ("one_wg_big", "large", 0), ("one_wg_big", "large", 1), ("lists", "large", 1)])
def test_padded_lists_beyond_their_capacity_are_cut_counted_and_stay_in_bounds(form, name, capp):
    """world 8, a per-pair capacity (HipBackend(halo_cap=...)) chosen from the reference so that at least one list overflows and at
    least one non-empty list does not (capp = 0 here: the median list length; and capp = 1): the count word is min(len, capp), the ids
    the ascending prefix, every word behind a list and behind the buffer keeps its sentinel, and sg_stats.halo_overflow grows by
    exactly the ids that did not fit — in the first window and again in a second one — and by nothing in a twin run of the same
    engines' window with room for every list.  (The rows of an overflowed window are unspecified and not compared.)"""
    world, case = 8, _case(name)
    ref = case.ref(0, world)
    capp = capp or _overflow_capp(ref, world)
    sizes = ref.pair_sizes()
    assert (sizes > capp).any() and ((sizes > 0) & (sizes <= capp)).any(), (capp, sizes)
    want = [ref.padded(r, capp)[2] for r in range(world)]
    assert sum(want) > 0
    with Shards(case, world, form, halo_cap=capp) as sh:
        assert sh.capp == capp and sh.overflow() == [0] * world
        for n in (1, 2):
            lists, _, nn = sh.window(case.windows[0], case.n_labels)
            assert nn == [ref.N] * world
            sh.check_lists(lists, ref)
            assert sh.overflow() == [n * w for w in want], (n, sh.overflow(), want)
    with Shards(case, world, form) as sh:
        lists, rows, _ = sh.window(case.windows[0], case.n_labels)
        sh.check_lists(lists, ref)
        assert sh.overflow() == [0] * world and rows.tobytes() == case.want[0][0].tobytes()


@pytest.mark.parametrize("cap_of", ["half", "one", "exact"])
def test_unpadded_lists_beyond_their_capacity_fill_in_owner_order(cap_of):
    """sg_halo_build with room for fewer ids than the shard needs (half of them; one; and exactly as many as fit): the owners' groups
    fill ids in owner order, counts[k] is what of owner k's group lies before `cap` (the clamp in k6_halo_build), ids[:sum(counts)] is
    the prefix of the concatenated reference lists and every word from `cap` on keeps its sentinel.  include/servicegraph.h promises
    the sg_stats.halo_overflow count for the padded calls only, and that is what happens: the unpadded call drops what does not fit
    WITHOUT counting it — its caller reads counts back and must compare their sum with what it expected (asserted here as 0 growth)."""
    world, case = 8, _case("t120")
    ref = case.ref(0, world)
    total = [sum(len(l) for l in ref.req(r)) for r in range(world)]
    cap = {"half": min(total) // 2, "one": 1, "exact": min(total)}[cap_of]
    assert 0 < cap <= min(total) and (cap_of == "exact" or cap < min(total))
    with Shards(case, world, "unpadded") as sh:
        lists, _, nn = sh.window(case.windows[0], case.n_labels, unpadded_cap=cap)
        assert nn == [ref.N] * world
        sh.check_lists(lists, ref, unpadded_cap=cap)
        for r in range(world):
            assert int(lists[r][0][:world].sum()) == cap
        assert sh.overflow() == [0] * world


# ---- e. pack and unpack as copies -----------------------------------------------------------------------------------------------
def _rc(call, *a):
    from alaz_amd import engine
    with pytest.raises(engine.ServiceGraphError) as ei:
        call(*a)
    return ei.value.rc


@pytest.mark.parametrize("world,capp", [(8, 1), (8, 7), (8, 1024), (3, 1), (3, 7), (3, 1024)])
def test_pack_and_unpack_copy_exactly_the_listed_rows(world, capp):
    """no window: a 2-layer engine whose layer buffers are the test's own tensors with a distinct bit pattern in every element, and
    hand-made lists — full rows (count = capp), a row with count 0 between two full ones, a row with count 1, node ids 0 and
    ncap - 1, stale ids behind every count.  halo_pack_padded: rows_out[r][i] = feat[l][list[r][1 + i]] bit for bit for i < count,
    every other word of rows_out and behind it keeps its sentinel.  halo_unpack_padded: the inverse, every row of the layer buffer
    that is not listed is unchanged.  The same for halo_pack / halo_unpack (n = 0, 1 and many), both layers; l = 0 and l > layers are
    refused with SG_EINVAL by all four calls."""
    import torch
    from alaz_amd import engine
    layers, nk = 2, 8000
    g = engine.ServiceGraph(max_known_nodes=nk, max_edges=1024, layers=layers, max_labels=1024, max_outbound_ips=72, rank=1, world=world,
                            max_batch=1 << 12, max_window_events=1 << 12)
    try:
        ncap = nk + 1024 + 72
        dev = torch.device("cuda", 0)
        st = torch.cuda.Stream(dev)
        rng = np.random.default_rng(capp * 16 + world)
        with torch.cuda.stream(st):
            pattern = lambda n, tag: torch.arange(n, dtype=torch.int32, device=dev) + (tag << 24)
            feat0 = [pattern(ncap * 64 + GUARD, 1 + l) for l in range(layers)]
            feat = [f.clone() for f in feat0]
            g.bind_buffers(0, 0, [f.data_ptr() for f in feat])
            # lists: row 0 full, row 1 empty, row 2 full, row 3 (world 8) one id, the rest a random count; ids distinct over the whole
            # buffer (unpack writes each once), 0 and ncap - 1 among them; stale in-range ids behind every count
            counts = [capp, 0, capp] + ([1] + [int(rng.integers(0, capp + 1)) for _ in range(world - 4)] if world > 3 else [])
            perm = rng.permutation(np.arange(1, ncap - 1))[: sum(counts)].tolist()
            perm[0] = 0; perm[-1] = ncap - 1
            lst = np.full((world, capp + 1), 5, dtype=np.int32)
            at = 0
            for r, c in enumerate(counts):
                lst[r, 0] = c; lst[r, 1:1 + c] = perm[at:at + c]; at += c
            d_lst = torch.from_numpy(lst).to(dev)
            for l in range(1, layers + 1):
                # pack
                rows = torch.full((world * capp * 64 + GUARD,), SENT, dtype=torch.int32, device=dev)
                g.halo_pack_padded(l, d_lst.data_ptr(), capp, rows.data_ptr(), st.cuda_stream)
                want = torch.full_like(rows, SENT)
                wv = want[: world * capp * 64].view(world, capp, 64); fv = feat0[l - 1][: ncap * 64].view(ncap, 64)
                for r, c in enumerate(counts):
                    if c: wv[r, :c] = fv[torch.from_numpy(lst[r, 1:1 + c].astype(np.int64)).to(dev)]
                assert torch.equal(rows, want), (l, "pack_padded")
                assert torch.equal(feat[l - 1], feat0[l - 1]) and torch.equal(d_lst.cpu(), torch.from_numpy(lst))
                # unpack
                rin = pattern(world * capp * 64 + GUARD, 8 + l)
                g.halo_unpack_padded(l, d_lst.data_ptr(), capp, rin.data_ptr(), st.cuda_stream)
                want = feat0[l - 1].clone()
                wf = want[: ncap * 64].view(ncap, 64); rv = rin[: world * capp * 64].view(world, capp, 64)
                for r, c in enumerate(counts):
                    if c: wf[torch.from_numpy(lst[r, 1:1 + c].astype(np.int64)).to(dev)] = rv[r, :c]
                assert torch.equal(feat[l - 1], want), (l, "unpack_padded")
                assert torch.equal(feat[2 - l], feat0[2 - l])                            # the other layer's buffer is untouched
                feat[l - 1].copy_(feat0[l - 1])
                # the unpadded pair: n = 0, 1, many
                for n in (0, 1, min(len(perm), 1000)):
                    ids = torch.tensor(perm[len(perm) - n:] + [5] * GUARD, dtype=torch.int32, device=dev)
                    rows = torch.full((n * 64 + GUARD,), SENT, dtype=torch.int32, device=dev)
                    g.halo_pack(l, ids.data_ptr(), n, rows.data_ptr(), st.cuda_stream)
                    want = torch.full_like(rows, SENT)
                    if n: want[: n * 64].view(n, 64)[:] = fv[ids[:n].long()]
                    assert torch.equal(rows, want), (l, n, "pack")
                    rin = pattern(n * 64 + GUARD, 12 + l)
                    g.halo_unpack(l, ids.data_ptr(), n, rin.data_ptr(), st.cuda_stream)
                    want = feat0[l - 1].clone()
                    if n: want[: ncap * 64].view(ncap, 64)[ids[:n].long()] = rin[: n * 64].view(n, 64)
                    assert torch.equal(feat[l - 1], want), (l, n, "unpack")
                    feat[l - 1].copy_(feat0[l - 1])
            for l in (0, layers + 1):
                rows = torch.full((world * capp * 64 + GUARD,), SENT, dtype=torch.int32, device=dev)
                assert _rc(g.halo_pack_padded, l, d_lst.data_ptr(), capp, rows.data_ptr(), st.cuda_stream) == engine.SG_EINVAL
                assert _rc(g.halo_unpack_padded, l, d_lst.data_ptr(), capp, rows.data_ptr(), st.cuda_stream) == engine.SG_EINVAL
                assert _rc(g.halo_pack, l, d_lst.data_ptr(), 1, rows.data_ptr(), st.cuda_stream) == engine.SG_EINVAL
                assert _rc(g.halo_unpack, l, d_lst.data_ptr(), 1, rows.data_ptr(), st.cuda_stream) == engine.SG_EINVAL
                st.synchronize()
                assert (rows == SENT).all() and all(torch.equal(a, b) for a, b in zip(feat, feat0))
    finally:
        g.close()
