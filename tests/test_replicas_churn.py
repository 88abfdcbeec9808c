"""The parameters of the churn test of the replica outliers (K25; tests/test_gpu_replicas.py runs the engine under them after
sg_set_replicas) give non-zero counts by the reference alone: the thinned churn windows of tests/traces.py are closed by the
oracle, its edges and their histograms are folded here into node rows, workload rows under the `blocks` map and node histograms —
sums by endpoint, as K9, K16 and K20 define them — and tests/replica_ref.py counts judged sides, outlier sides of every kind and
non-members.  No engine and no GPU."""
import numpy as np

from alaz_amd import engine, weights
from alaz_amd.engine import NODE_DTYPE
from oracle import pyoracle
from tests.helpers import CLOCK, G, HostShim
from tests.replica_ref import CHURN_COUNTS, CHURN_PARAMS, CHURN_STEP, CHURN_WINDOWS, replica_ref, tally
from tests.traces import churn  # noqa: F401  (the fixture)

NO = engine.NO_GROUP
M64 = (1 << 64) - 1


class _Quiet:
    upsert_pod = upsert_service = delete_pod = delete_service = staticmethod(lambda *a: None)


def _rows(table, order):
    r = np.zeros(len(table), dtype=NODE_DTYPE)
    h = np.zeros((len(table), 2, 16), dtype=np.uint64)
    for k, ref in enumerate(sorted(table, key=order)):
        r[k]["ref"] = ref
        for hs, side in ((0, "out"), (1, "in")):
            c, e, s, b = table[ref][side]
            r[k][side + "_count"], r[k][side + "_err"], r[k][side + "_sum_ns"] = c, e, s
            h[k, hs] = b
    return r, h


def _fold(edges, hist, ids, gmap):
    """node rows, workload rows and node histograms from the oracle's edges: a KNOWN ref is the shim's id of the UID, an outbound
    end a LABEL ref of its own (no member either way)"""
    outbound = {}

    def ref(kind, uid):
        if kind in ("pod", "service"):
            return ids[uid]
        return 1 << 30 | outbound.setdefault(uid, len(outbound))

    def key(r):
        return G(int(gmap[r])) if r < len(gmap) and int(gmap[r]) != NO else r
    acc, wacc = {}, {}
    for e, bins in zip(edges, hist):
        f, t = ref(e.from_type.decode(), e.from_uid.decode()), ref(e.to_type.decode(), e.to_uid.decode())
        for table, kf, kt in ((acc, f, t), (wacc, key(f), key(t))):
            for k, side in ((kf, "out"), (kt, "in")):
                a = table.setdefault(k, {s: [0, 0, 0, [0] * 16] for s in ("in", "out")})[side]
                a[0] += e.row.count; a[1] += e.row.err_count; a[2] = (a[2] + e.row.sum_ns) & M64
                a[3] = [x + int(y) for x, y in zip(a[3], bins)]
    nodes, nhist = _rows(acc, lambda r: r)
    wrows, _ = _rows(wacc, lambda r: (0, r & 0x3FFFFFFF) if r >> 30 == 3 else (1, r))   # the groups first, as K16 orders them
    return nodes, nhist, wrows


def test_the_churn_parameters_are_not_vacuous_by_the_reference_alone(churn):
    topo, labels, wins = churn
    mk = topo.n_nodes + 8
    sh = HostShim(); sh.apply(_Quiet(), topo.k8s_ops())
    kinds = np.zeros(mk, np.uint8)
    kinds[:len(sh.kind)] = [1 if x == "pod" else 2 for x in sh.kind]
    gmap = np.full(mk, NO, np.uint32)
    gmap[:topo.n_pods] = np.arange(topo.n_pods) // 7                  # gpu_scaffold._map("blocks", ...)
    assert (kinds[:topo.n_pods] == 1).all()
    W = weights.make_weights(2)
    t = None
    for w in wins[:CHURN_WINDOWS]:
        o = pyoracle.Oracle(*CLOCK); o.apply_ops(topo.k8s_ops())
        o.packed(np.ascontiguousarray(w[::CHURN_STEP]), labels); o.window_close(W, 2)
        nodes, hist, wrows = _fold(o.edges(), o.edge_hist(), sh.ids, gmap)
        assert len(nodes) > 100 and int(nodes["in_count"].sum()) == int(nodes["out_count"].sum()) > 1000
        pods, groups = replica_ref(nodes, wrows, hist, gmap, kinds, CHURN_PARAMS)
        assert int(groups[:, 1].sum() + groups[:, 5].sum()) == tally(pods)["judged"]
        t = tally(pods, t)
        o.close()
    print("churn by the reference alone:", t)
    assert all(v > 0 for v in t.values()), t
    assert t["judged"] > 100 and min(t["err"], t["lat"], t["tail"]) > 10 and t["non_members"] > 100   # not by a hair
    assert t == CHURN_COUNTS                                          # what the GPU test expects of the engine's own rows
