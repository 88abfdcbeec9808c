"""The Python side's twins of the header's structs and constants, and the C source that holds them to include/servicegraph.h by the
compiler (tests/test_abi.py; the stages' own tests check their structs through the same source)."""
import ctypes as C

import numpy as np

from alaz_amd import engine, replay

#: the header's name of every struct the Python side declares a twin of (a ctypes.Structure or a numpy dtype)
LAYOUTS = {
    "sg_config": engine.SgConfig, "sg_geometry": engine.SgGeometry, "sg_stats": engine.SgStats,
    "sg_trend_params": engine.SgTrendParams, "sg_trend_stats": engine.SgTrendStats, "sg_vanished_params": engine.SgVanishedParams,
    "sg_rank_params": engine.SgRankParams, "sg_incident_params": engine.SgIncidentParams, "sg_track_params": engine.SgTrackParams,
    "sg_track_stats": engine.SgTrackStats, "sg_group_params": engine.SgGroupParams,
    "sg_event": replay.EVENT_DTYPE, "sg_edge_out": replay.EDGE_OUT_DTYPE,
    "sg_edge_trend": engine.TREND_DTYPE, "sg_trend_entry": engine.TREND_ENTRY_DTYPE, "sg_edge_vanished": engine.VANISHED_DTYPE,
    "sg_node_out": engine.NODE_DTYPE, "sg_node_trend": engine.NODE_TREND_DTYPE, "sg_node_rank": engine.RANK_DTYPE,
    "sg_incident_out": engine.INCIDENT_DTYPE, "sg_incident_track": engine.TRACK_DTYPE, "sg_track_entry": engine.TRACK_ENTRY_DTYPE,
    "sg_group_edge": engine.GROUP_EDGE_DTYPE,
}
#: every constant engine.py and replay.py copy from the header
CONSTANTS = {
    **{"SG_" + n: getattr(engine, "SG_" + n) for n in ("OK", "EINVAL", "ENOMEM", "ENODEV", "ENOSPC", "EAGAIN", "ESTATE")},
    "SG_ABI_VERSION": engine.ABI_VERSION, "SG_SELECT_MAX_K": engine.SELECT_MAX_K,
    "SG_F_IN": engine.F_IN, "SG_F_HID": engine.F_HID, "SG_F_EDGE": engine.F_EDGE,
    "SG_NODE_STAT_SUM_WORDS": engine.STAT_SUM_WORDS, "SG_NODE_STAT_MAX_WORDS": engine.STAT_MAX_WORDS,
    "SG_REF_KNOWN": engine.REF_KNOWN, "SG_REF_LABEL": engine.REF_LABEL, "SG_REF_OBIP": engine.REF_OBIP, "SG_REF_GROUP": engine.REF_GROUP,
    "SG_NO_INCIDENT": engine.NO_INCIDENT, "SG_NO_TRACK": engine.NO_TRACK, "SG_NO_GROUP": engine.NO_GROUP,
    "SG_TRACK_NEW": engine.TRACK_NEW, "SG_TRACK_SPLIT": engine.TRACK_SPLIT, "SG_TRACK_MERGED": engine.TRACK_MERGED,
    **{"SG_SEL_" + k.upper(): v for k, v in engine.SEL_BY.items()}, **{"SG_NSEL_" + k.upper(): v for k, v in engine.NSEL_BY.items()},
    **{"SG_RANK_SEED_" + k.upper(): v for k, v in engine.RANK_SEED.items()},
    "SG_CFG_EDGE_HISTOGRAM": engine.CFG_EDGE_HISTOGRAM, "SG_CFG_NO_WARM": engine.CFG_NO_WARM, "SG_CFG_WARM": engine.CFG_WARM,
    "SG_HIST_BINS": replay.HIST_BINS, **{"SG_EV_" + n: getattr(replay, "EV_" + n) for n in ("TLS", "REVERSE", "CONSUME", "ALIVE")},
    **{"SG_PROTO_" + n: getattr(replay, "PROTO_" + n) for n in ("HTTP", "AMQP", "POSTGRES", "HTTP2", "REDIS", "KAFKA", "MYSQL", "MONGO")},
}


def _fields(t):
    """(name, offset, size, kind 'u' / 'i' / 'f', elements or 0) of every field of a ctypes.Structure or a numpy dtype"""
    if isinstance(t, np.dtype):
        for name, (dt, off) in ((n, t.fields[n][:2]) for n in t.names):
            yield name, off, dt.itemsize, dt.base.kind, int(np.prod(dt.shape)) if dt.shape else 0
    else:
        for name, ct in t._fields_:
            el = getattr(ct, "_length_", 0)
            code = (ct._type_ if el else ct)._type_
            yield name, getattr(t, name).offset, getattr(t, name).size, "f" if code in "fd" else "i" if code in "bhilq" else "u", el


def layout_check_source() -> str:
    """A C11 translation unit that compiles only when the header agrees with the Python declarations: one _Static_assert per struct
    size, three per field (its offset by NAME, its size, and that it is a float, a signed or an unsigned integer) and one per constant."""
    out = ["#include <stddef.h>", '#include "servicegraph.h"',
           "#define KIND(x) _Generic((x), float: 'f', double: 'f', int8_t: 'i', int16_t: 'i', int32_t: 'i', int64_t: 'i', default: 'u')"]
    for ctype, t in LAYOUTS.items():
        size = t.itemsize if isinstance(t, np.dtype) else C.sizeof(t)
        out.append(f'_Static_assert(sizeof({ctype}) == {size}, "sizeof({ctype}) is not {size}");')
        for name, off, fsize, kind, el in _fields(t):
            m, what = f"(({ctype}*)0)->{name}", f"{ctype}.{name}"
            out.append(f'_Static_assert(offsetof({ctype}, {name}) == {off}, "{what} is not at offset {off}");')
            out.append(f'_Static_assert(sizeof({m}) == {fsize}, "{what} is not {fsize} bytes");')
            out.append(f"_Static_assert(KIND({m}{'[0]' if el else ''}) == '{kind}', \"{what} is not of kind '{kind}'\");")
    for name, v in CONSTANTS.items():
        out.append(f'_Static_assert((long long)({name}) == {int(v)}LL, "{name} is not {int(v)}");')
    return "\n".join(out) + "\n"
