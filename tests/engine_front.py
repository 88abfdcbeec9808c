"""The recording stand-in for libservicegraph.so that the CPU tests of the ctypes front end (alaz_amd/engine.py) talk to: a ServiceGraph
built by hand, every C call recorded with its decoded arguments (tests/test_engine_front.py says how they are decoded), output buffers
filled with a known pattern.  A stage's test module extends ABI with its own functions: g = abi_fixture(NEW_ABI)."""
import ctypes as C
import functools
import sys

import numpy as np
import pytest

from alaz_amd import engine
from alaz_amd.replay import EDGE_OUT_DTYPE, EVENT_DTYPE

U4 = np.dtype("<u4")
HIST = np.dtype((np.uint32, 16))         # one row of sg_window_hist: 16 bins
INF = float("-inf")


class Out:
    """a caller-owned buffer of `dtype` rows the library writes; its capacity is the argument at position `cap`"""
    def __init__(self, dtype, cap): self.itemsize, self.cap = np.dtype(dtype).itemsize, cap


class In:
    """a buffer of `dtype` the library reads; its length is the argument at position `count`"""
    def __init__(self, dtype, count): self.dtype, self.count = np.dtype(dtype), count


H, I, F, O, S, SO = "handle", "int", "float", "scalar out", "struct in", "struct out"
_COUNTED = lambda dt: [H, Out(dt, 2), I, O]                      # f(h, out, cap, *n)
_INDEXED = lambda dt: [H, In(U4, 2), I, Out(dt, 4), I, O]        # f(h, index, n_index, out, cap, *n)
#: the arguments of every C function these tests reach, as include/servicegraph.h declares them
ABI = {
    "sg_last_error": [H], "sg_ingest": [H, In(EVENT_DTYPE, 2), I],
    **{f: [H, S] for f in ("sg_set_trend", "sg_set_node_trend", "sg_set_vanished", "sg_set_rank", "sg_set_incidents", "sg_set_tracks",
                           "sg_set_groups")},
    "sg_window_nodes": _COUNTED(engine.NODE_DTYPE), "sg_window_incidents": _COUNTED(engine.INCIDENT_DTYPE),
    "sg_trend_entries": _COUNTED(engine.TREND_ENTRY_DTYPE), "sg_node_trend_entries": _COUNTED(engine.TREND_ENTRY_DTYPE),
    "sg_window_vanished": _COUNTED(engine.VANISHED_DTYPE), "sg_window_outbound_ips": _COUNTED(U4), "sg_window_hist": _COUNTED(HIST),
    "sg_window_incident_tracks": _COUNTED(engine.TRACK_DTYPE), "sg_window_tracks_ended": _COUNTED(engine.TRACK_ENTRY_DTYPE),
    "sg_track_entries": _COUNTED(engine.TRACK_ENTRY_DTYPE), "sg_window_groups": _COUNTED(engine.GROUP_EDGE_DTYPE),
    "sg_window_group_perm": _COUNTED(U4), "sg_window_read": _COUNTED(EDGE_OUT_DTYPE), "sg_flush_end": _COUNTED(EDGE_OUT_DTYPE),
    "sg_flush_window": [H, I, Out(EDGE_OUT_DTYPE, 3), I, O],
    "sg_window_trend": _INDEXED(engine.TREND_DTYPE), "sg_window_node_trend": _INDEXED(engine.NODE_TREND_DTYPE),
    "sg_window_rank": _INDEXED(engine.RANK_DTYPE), "sg_window_node_incident": _INDEXED(U4), "sg_window_row_group": _INDEXED(U4),
    "sg_flush_window_top": [H, I, I, F, Out(EDGE_OUT_DTYPE, 6), Out(U4, 6), I, O, O],
    "sg_flush_window_top_by": [H, I, I, I, F, Out(EDGE_OUT_DTYPE, 7), Out(U4, 7), I, O, O],
    "sg_flush_end_top": [H, I, F, Out(EDGE_OUT_DTYPE, 5), Out(U4, 5), I, O, O],
    "sg_flush_end_top_by": [H, I, I, F, Out(EDGE_OUT_DTYPE, 6), Out(U4, 6), I, O, O],
    "sg_window_select": [H, I, F, I, I, I, I, I], "sg_window_select_by": [H, I, I, F, I, I, I, I, I],
    "sg_window_nodes_top": [H, I, I, F, Out(engine.NODE_DTYPE, 6), Out(U4, 6), I, O, O],
    "sg_window_nodes_select": [H, I, I, F, I, I, I, I, I],
    "sg_window_rank_top": [H, I, F, Out(engine.NODE_DTYPE, 6), Out(engine.RANK_DTYPE, 6), Out(U4, 6), I, O, O],
    "sg_window_rank_select": [H, I, F, I, I, I, I, I],
    **{f: [H, O] for f in ("sg_window_trend_buffer", "sg_window_node_trend_buffer", "sg_window_rank_buffer", "sg_window_rows_buffer")},
    "sg_window_vanished_buffer": [H, O, O], "sg_window_nodes_buffer": [H, O, O],
    "sg_window_incidents_buffer": [H, O, O, O], "sg_window_tracks_buffer": [H, O, O, O],
    "sg_window_groups_buffer": [H, O, O, O, O], "sg_window_buffers": [H, O, O, O, O], "sg_window_feat_buffer": [H, I, O, O],
    **{f: [H, SO] for f in ("sg_stats_get", "sg_trend_stats_get", "sg_node_trend_stats_get", "sg_track_stats_get")},
}


def pattern(dtype, rows):
    """what the stand-in writes into an output buffer: every byte of row j is (j + 1) & 255"""
    dtype = np.dtype(dtype)
    raw = ((np.arange(rows) + 1) & 255).astype(np.uint8).repeat(dtype.itemsize)
    return np.frombuffer(raw.tobytes(), dtype=dtype.base).reshape((rows,) + dtype.shape)


class Numpy:
    """numpy as engine.py sees it, remembering where every array it hands out lies"""
    def __init__(self, spans): self._spans = spans

    def __getattr__(self, name):
        f = getattr(np, name)
        if name not in ("zeros", "empty", "ascontiguousarray"):
            return f

        def made(*a, **kw):
            arr = f(*a, **kw)
            self._spans.append((arr.ctypes.data, arr.nbytes, arr))      # (the reference keeps the address from being reused)
            return arr
        return made


class Lib:
    """The recording stand-in.  script[name] = dict(rc=return code, out=[values of the scalar out-parameters in order],
    fields={stats field: value}, text=sg_last_error's bytes); a function without a script returns 0 and writes zeros.  Every
    output buffer gets min(out[0], cap) rows of pattern()."""
    def __init__(self, h, spans):
        self.h, self.spans, self.calls, self.script = h, spans, [], {}

    def __getattr__(self, name):
        if name not in ABI:
            raise AttributeError(name)
        return functools.partial(self._call, name)

    def _inside(self, addr, nbytes):
        return any(a <= addr and addr + nbytes <= a + n for a, n, _ in self.spans)

    def _call(self, name, *args):
        kinds, s = ABI[name], self.script.get(name, {})
        assert len(args) == len(kinds), (name, args)
        outs = list(s.get("out", ()))
        have, nxt, dec = (outs[0] if outs else 0), iter(outs), []
        for a, k in zip(args, kinds):
            if k is H:
                dec.append("h" if a is self.h else repr(a))
            elif k is I:
                assert a is None or type(a) is int, (name, a)
                dec.append(a)
            elif k is F:
                dec.append(float(a))
            elif k is O:
                a._obj.value = next(nxt, 0)
                dec.append("out")
            elif k is S:
                dec.append(None if a is None else bytes(a._obj))
            elif k is SO:
                for f, v in s.get("fields", {}).items():
                    setattr(a._obj, f, v)
                dec.append("out:" + type(a._obj).__name__)
            elif isinstance(k, Out):
                if a is None:
                    dec.append(None)
                    continue
                cap = args[k.cap]
                ok = type(a) is int and a != 0 and self._inside(a, cap * k.itemsize)
                dec.append("buf" if ok else f"BAD buffer {a!r} for {cap} x {k.itemsize}")
                if ok:
                    C.memmove(a, pattern(np.dtype((np.uint8, k.itemsize)), min(have, cap)).tobytes(), min(have, cap) * k.itemsize)
            elif isinstance(k, In):
                if a is None:
                    dec.append(None)
                    continue
                n = args[k.count]
                ok = type(a) is int and a != 0 and self._inside(a, n * k.dtype.itemsize)
                dec.append(("in", np.frombuffer(C.string_at(a, n * k.dtype.itemsize), dtype=k.dtype).tolist()) if ok
                           else f"BAD buffer {a!r} for {n} x {k.dtype.itemsize}")
        self.calls.append((name, *dec))
        return s.get("text", b"") if name == "sg_last_error" else s.get("rc", 0)

    def take(self):
        c, self.calls = self.calls, []
        return c


def same(a, dtype, want):
    assert isinstance(a, np.ndarray) and a.dtype == np.dtype(dtype).base and a.shape == want.shape, (a.dtype, a.shape)
    assert a.tobytes() == want.tobytes(), (a.tolist()[:4], want.tolist()[:4])


def abi_fixture(new_abi):
    """the fixture `g` of a stage's test module: the hand-built ServiceGraph over a stand-in that also knows the stage's functions"""
    @pytest.fixture
    def g(monkeypatch):
        monkeypatch.setattr(sys.modules[__name__], "ABI", {**ABI, **new_abi})
        spans = []
        monkeypatch.setattr(engine, "np", Numpy(spans))
        g = object.__new__(engine.ServiceGraph)
        g._h = C.c_void_p(0x5A5A)
        g.layers, g.max_edges, g.max_batch, g.rank, g.world = 2, 100, 1 << 16, 0, 1
        g._l = Lib(g._h, spans)
        yield g
        g._h = None
    return g
