"""The reference of the replica outliers (K25; include/servicegraph.h, "replica outliers"): plain Python over a window's node rows
and workload rows (engine.NODE_DTYPE), the node rows' K20 histograms ((n, 2, 16) u64, out side then in side; None without tails),
the group map and the kinds per KNOWN id, and the parameters.  Python integers only — wrapping is spelled out where the definition
wraps.  Not a test module."""
import numpy as np

WORDS, GROUP_WORDS = 12, 8
NONE = 0xFFFFFFFF
NO_GROUP = 0xFFFFFFFF
M64 = (1 << 64) - 1
KNOWN, GROUP = 0, 3
POD, SERVICE = 1, 2
MEMBER, JUDGED, ERR, LAT, TAIL = 1, 2, 4, 8, 16                      # the in side's flags; the out side's are << 4
SIDES = ("in", "out")                                                 # the row's side order; K20's tables hold them as (out, in)
BY = dict(err=0, lat=1, tail=2, share=3)
#: the parameters of the churn tests (tests/traces.py thinned to an eighth, seven replicas a workload): a pod sends a dozen requests a
#: window and receives a few.  tests/test_replicas_churn.py holds on the CPU that the reference alone finds judged sides, outliers of
#: every kind and non-members under them; tests/test_gpu_replicas.py runs the engine under the same ones
CHURN_PARAMS = dict(min_replicas=3, min_requests=4, min_err_excess_q20=1 << 15, min_lat_ratio_q10=1536, tail_permille=900, min_tail_bins=1)
CHURN_STEP, CHURN_WINDOWS = 8, 6
#: ... and what the reference counts over those windows, from the oracle's edges on the CPU and from the engine's rows alike
CHURN_COUNTS = dict(non_members=1137, judged=1388, err=269, lat=195, tail=349)
DEFAULTS = dict(min_replicas=3, min_requests=20, min_err_excess_q20=20972, min_lat_ratio_q10=2048, tail_permille=0, min_tail_bins=2)


def resolve(params):
    """the parameters in force: a 0 (or an absent one) is the stage's default"""
    return {k: int(params.get(k, 0)) or d for k, d in DEFAULTS.items()}


def x_err(e, c):
    return (min(e, c) << 20) // c


def mean(s, c):
    return min(s // c, 1 << 52)


def qbin(h, permille):
    """the first bin whose cumulative count reaches K20's rank, 15 when none does, 0 without requests"""
    total = sum(h)
    if total == 0:
        return 0
    rank = max(1, -(-total * permille // 1000))
    cum = 0
    for b, x in enumerate(h):
        cum += x
        if cum >= rank:
            return b
    return 15


def members(nodes, wrows, gmap, kinds):
    """per node row the workload row it is a member of, None for a non-member"""
    at = {int(r): k for k, r in enumerate(wrows["ref"].tolist())}
    out = []
    for ref in nodes["ref"].tolist():
        t, v = ref >> 30, ref & 0x3FFFFFFF
        w = None
        if t == KNOWN and v < len(gmap) and int(kinds[v]) == POD and int(gmap[v]) != NO_GROUP:
            w = at.get(GROUP << 30 | int(gmap[v]))
        out.append(w)
    return out


def side_of(row, side, hist, v):
    """(c, e, S, h) of side `side` ("in" / "out") of node row v"""
    h = [int(x) for x in hist[v][1 if side == "in" else 0]] if hist is not None else [0] * 16
    return int(row[side + "_count"]), int(row[side + "_err"]), int(row[side + "_sum_ns"]), h


def member_sums(nodes, wrows, hist, gmap, kinds):
    """{workload row: {side: [R, C, E, T, H]}} over the members, T wrapping"""
    sums = {}
    for v, w in enumerate(members(nodes, wrows, gmap, kinds)):
        if w is None:
            continue
        s = sums.setdefault(w, {sd: [0, 0, 0, 0, [0] * 16] for sd in SIDES})
        for sd in SIDES:
            c, e, S, h = side_of(nodes[v], sd, hist, v)
            a = s[sd]
            a[0] += c > 0; a[1] += c; a[2] += e; a[3] = (a[3] + S) & M64
            a[4] = [x + y for x, y in zip(a[4], h)]
    return sums


def judge(c, e, S, h, R, C, E, T, H, p):
    """(flags of the in side's bits, err_excess_q20, lat_ratio_q10, share_q10, tail_pod, tail_peers) of one side, p resolved"""
    if not (c >= p["min_requests"] and C - c >= p["min_requests"] and R >= p["min_replicas"]):
        return 0, 0, 0, 0, 0, 0
    excess = x_err(e, c) - x_err(E - e, C - c)
    ratio = min(mean(S, c) * 1024 // max(mean((T - S) & M64, C - c), 1), NONE)
    share = min(min(c, 1 << 53) * 1024 // max(C // R, 1), NONE)
    f = JUDGED | (ERR if excess >= p["min_err_excess_q20"] else 0) | (LAT if ratio >= p["min_lat_ratio_q10"] else 0)
    tp = tq = 0
    if p["tail_permille"]:
        tp, tq = qbin(h, p["tail_permille"]), qbin([x - y for x, y in zip(H, h)], p["tail_permille"])
        if tp - tq >= p["min_tail_bins"]:
            f |= TAIL
    return f, excess, ratio, share, tp, tq


def replica_ref(nodes, wrows, hist, gmap, kinds, params):
    """the pod rows (n, 12) u32 and the workload rows (m, 8) u32 of one window"""
    p = resolve(params)
    if not p["tail_permille"]:
        hist = None
    mem = members(nodes, wrows, gmap, kinds)
    sums = member_sums(nodes, wrows, hist, gmap, kinds)
    pods = np.zeros((len(nodes), WORDS), np.uint32)
    groups = np.zeros((len(wrows), GROUP_WORDS), np.uint32)
    groups[:, 3] = groups[:, 7] = NONE
    for w, s in sums.items():
        for i, sd in enumerate(SIDES):
            groups[w, 4 * i] = s[sd][0]
    for v, w in enumerate(mem):
        if w is None:
            pods[v, 0] = NONE
            continue
        flags = MEMBER
        pods[v, 0] = w
        for i, sd in enumerate(SIDES):
            c, e, S, h = side_of(nodes[v], sd, hist, v)
            R, C, E, T, H = sums[w][sd]
            f, excess, ratio, share, tp, tq = judge(c, e, S, h, R, C, E, T, H, p)
            pods[v, 2 + 5 * i: 7 + 5 * i] = [excess & NONE, ratio, share, tp | tq << 8, R]
            flags |= f << (4 * i)
            if f & JUDGED:
                groups[w, 4 * i + 1] += 1
            if f & (ERR | LAT | TAIL):
                groups[w, 4 * i + 2] += 1
                groups[w, 4 * i + 3] = min(int(groups[w, 4 * i + 3]), v)
        pods[v, 1] = flags
    return pods, groups


def tally(pods, t=None):
    """pod rows counted into t: non-members, judged sides and the outlier sides of each kind"""
    t = dict(non_members=0, judged=0, err=0, lat=0, tail=0) if t is None else t
    for r in pods.tolist():
        t["non_members"] += r[0] == NONE
        for i in range(2):
            s = r[1] >> (4 * i)
            t["judged"] += bool(s & JUDGED); t["err"] += bool(s & ERR); t["lat"] += bool(s & LAT); t["tail"] += bool(s & TAIL)
    return t


def replica_values(pods, by, side):
    """the selection's key per pod row: 0 for a side that is not judged"""
    i = SIDES.index(side)
    out = []
    for r in pods.tolist():
        q = r[2 + 5 * i: 7 + 5 * i]
        if not r[1] & (JUDGED << (4 * i)):
            out.append(0)
        elif by == "err":
            out.append(q[0] if q[0] < 1 << 31 else 0)
        elif by == "lat":
            out.append(q[1])
        elif by == "tail":
            out.append(max((q[3] & 255) - (q[3] >> 8 & 255), 0))
        else:
            out.append(q[2])
    return out


def ref_select_replicas(pods, by, side, k, min_value):
    """the node positions sg_window_replicas_top selects: keys >= max(min_value, 1), descending, ties by position, the first k; k = 0:
    all of them, in row order"""
    vals = replica_values(pods, by, side)
    cand = [i for i, x in enumerate(vals) if x >= max(min_value, 1)]
    if k == 0:
        return np.array(cand, dtype=np.int64)
    cand.sort(key=lambda i: (-vals[i], i))
    return np.array(cand[:k], dtype=np.int64)
