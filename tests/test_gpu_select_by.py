"""K7 by a trend key (sg_flush_window_top_by / sg_flush_end_top_by / sg_window_select_by): the selected rows against a numpy selection
(tests/select_by_ref.py) over a TWIN engine's plain flush plus its window_trend().  A selection moves rows and computes nothing, so
every comparison is exact: row bytes, indices and counts."""

import numpy as np
import pytest

from alaz_amd import engine, replay
from tests.gpu_scaffold import _feed, _hip, _trend_engine as _engine
from tests.select_by_ref import ref_select_by
from tests.traces import trend_churn as churn  # noqa: F401

pytestmark = pytest.mark.gpu

ME = 1 << 15
PARAMS = dict(shift=3, warmup=2, ttl=3)
NEG_INF = float("-inf")
MAXK = engine.SELECT_MAX_K


def _twins(topo, labels, **kw):
    a, b = _engine(topo, labels, **kw), _engine(topo, labels, **kw)
    a.set_trend(**PARAMS); b.set_trend(**PARAMS)
    return a, b


def _check(sel, idx, ne, want, tr, by, k, mv):
    pos = ref_select_by(want, tr, by, k, mv)
    assert ne == len(want)
    assert np.array_equal(idx, pos[: len(idx)]) and len(idx) == min(len(pos), k if k else len(pos))
    assert sel.tobytes() == want[pos[: len(idx)]].tobytes()
    return len(pos)


@pytest.mark.parametrize("by", ["lat_dev", "err_dev", "new"])
def test_selection_by_each_key(churn, by):
    topo, labels, wins = churn
    a, b = _twins(topo, labels)
    cases = [(0, NEG_INF), (1, NEG_INF), (1000, NEG_INF), (MAXK, NEG_INF), (0, 0.5), (1000, 1.0), (MAXK, -0.0), (0, 3.0),
             (1, 0.0), (1000, -2.0), (0, float("nan")), (MAXK, 0.25)]
    sizes = []
    for (k, mv), w in zip(cases, wins):
        _feed(a, w); _feed(b, w)
        sel, idx, ne = a.flush_window_top(k, mv, by=by)
        want = b.flush_window(); tr = b.window_trend()
        sizes.append(_check(sel, idx, ne, want, tr, by, k, mv))
        assert a.window_trend(index=idx).tobytes() == tr[idx].tobytes()   # the positions go straight to sg_window_trend
        assert a.trend_entries().tobytes() == b.trend_entries().tobytes()
    assert sizes[0] > 1000 and min(sizes[:4]) > 0


def test_by_score_is_the_plain_selection(churn):
    topo, labels, wins = churn
    a, b = _twins(topo, labels)
    for k, w in zip((0, 1000, MAXK), wins[:3]):
        _feed(a, w); _feed(b, w)
        x = a.flush_window_top(k, 0.3 if k == 0 else NEG_INF, by="score")
        y = b.flush_window_top(k, 0.3 if k == 0 else NEG_INF)
        assert x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes() and x[2] == y[2]


@pytest.mark.parametrize("variant", [1, 2])
def test_split_flush_and_variants(churn, variant):
    topo, labels, wins = churn
    a, b = _twins(topo, labels, variant=variant, layers=1)
    for i, w in enumerate(wins[:6]):
        _feed(a, w); _feed(b, w)
        k, by = (1000, "lat_dev") if i % 2 else (0, "new")
        a.flush_begin()
        sel, idx, ne = a.flush_end_top(k, -1.0, by=by)
        want = b.flush_window(); tr = b.window_trend()
        _check(sel, idx, ne, want, tr, by, k, -1.0)
        st_a, st_b = a.stats(), b.stats()
        assert (st_a.windows, st_a.last_window_edges) == (st_b.windows, st_b.last_window_edges)


def test_cap_below_the_selection(churn):
    topo, labels, wins = churn
    a, b = _twins(topo, labels)
    for w in wins[:5]:
        _feed(a, w); _feed(b, w)
        sel, idx, ne = a.flush_window_top(0, NEG_INF, by="err_dev", cap=100)
        want = b.flush_window(); tr = b.window_trend()
        pos = ref_select_by(want, tr, "err_dev", 0, NEG_INF)
        assert len(pos) > 100 and np.array_equal(idx, pos[:100]) and sel.tobytes() == want[pos[:100]].tobytes()


@pytest.mark.parametrize("in_flight", [1, 2])
def test_window_select_by_on_the_device(churn, in_flight):
    import torch
    topo, labels, wins = churn
    g, b = _engine(topo, labels, windows_in_flight=in_flight), _engine(topo, labels)
    g.set_trend(**PARAMS); b.set_trend(**PARAMS)
    hip = _hip()
    dev = [torch.from_numpy(np.ascontiguousarray(w).view(np.uint8).reshape(-1)).cuda() for w in wins[:6]]
    cap = 2000
    d_out = torch.zeros(cap * 64, dtype=torch.uint8, device="cuda")
    d_idx = torch.zeros(cap, dtype=torch.int32, device="cuda")
    d_n = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for i, w in enumerate(wins[:6]):
        by, k, mv = (("lat_dev", 1000, NEG_INF), ("new", 0, 0.0), ("err_dev", MAXK, NEG_INF))[i % 3]
        _feed(b, w); want = b.flush_window(); tr = b.window_trend()
        g.ingest_device(dev[i].data_ptr(), len(w), 0)
        g.window_run(0)
        g.window_select(k, mv, d_out.data_ptr(), d_idx.data_ptr(), cap, d_n.data_ptr(), 0, by=by)
        torch.cuda.synchronize()
        pos = ref_select_by(want, tr, by, k, mv)
        n_sel = int(d_n.item())
        assert n_sel == len(pos) > 0
        m = min(n_sel, cap)
        assert np.array_equal(d_idx.cpu().numpy()[:m].astype(np.uint32), pos[:m])
        assert d_out.cpu().numpy()[: m * 64].tobytes() == want[pos[:m]].tobytes()


def test_errors_come_before_any_window_is_closed(churn):
    topo, labels, wins = churn
    g = _engine(topo, labels)
    _feed(g, wins[0])
    for by in ("lat_dev", "err_dev", "new"):
        with pytest.raises(engine.ServiceGraphError) as ei:
            g.flush_window_top(10, by=by)                            # the trend is off
        assert ei.value.rc == engine.SG_ESTATE
    assert g._l.sg_flush_window_top_by(g._h, 0, 4, 10, 0.0, None, None, 0, None, None) == engine.SG_EINVAL
    assert g._l.sg_flush_window_top_by(g._h, 0, 1, MAXK + 1, 0.0, None, None, 0, None, None) == engine.SG_EINVAL
    assert g.stats().windows == 0                                    # nothing was closed
    with pytest.raises(ValueError):
        g.flush_window_top(10, by="p99")
    g.set_trend(**PARAMS)
    sel, idx, ne = g.flush_window_top(0, NEG_INF, by="new")          # the window fed before is still there: a fresh baseline,
    assert g.stats().windows == 1 and ne > 0                         # every live row is new
    assert len(idx) == int((sel["count"] > 0).sum()) > 0
    _feed(g, wins[1])
    g.flush_begin()
    assert g._l.sg_flush_end_top_by(g._h, 7, 10, 0.0, None, None, 0, None, None) == engine.SG_EINVAL
    sel, idx, ne = g.flush_end_top(10, by="lat_dev")                  # the flush is still open: ended here
    assert ne > 0 and len(sel) == 10 and g.stats().windows == 2
