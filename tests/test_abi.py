"""CPU tests of the drop-in boundary: the C-ABI library builds for gfx950, loads, exports every
symbol include/servicegraph.h declares, and refuses to run without a GPU (no CPU fallback)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from alaz_amd import build, engine, replay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    h = open(os.path.join(ROOT, "include", "servicegraph.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    return sorted(set(re.findall(r"\b(sg_[a-z0-9_]+)\s*\(", h)))


def test_header_and_binding_declare_the_same_symbols():
    assert _declared() == sorted(engine.EXPORTS)


def test_library_builds_loads_and_exports_every_symbol(engine_lib):
    for name in _declared():
        assert hasattr(engine_lib, name), name
    assert engine_lib.sg_abi_version() == engine.ABI_VERSION == 6
    from alaz_amd import weights
    assert engine_lib.sg_weights_count(1) == weights.weights_count(1) == 12993
    assert engine_lib.sg_weights_count(2) == weights.weights_count(2)
    assert engine_lib.sg_hash32(12345) == int(replay.hash32(np.array([12345], dtype=np.uint32))[0])


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


def test_struct_layouts_match_the_header(tmp_path):
    assert C.sizeof(engine.SgConfig) == 88 and C.sizeof(engine.SgStats) == 184 and C.sizeof(engine.SgGeometry) == 52
    assert engine.SgConfig.struct_size.offset == 0 and engine.SgConfig.abi_version.offset == 4 and engine.SgConfig.max_edges.offset == 32
    assert replay.EVENT_DTYPE.itemsize == 32 and replay.EDGE_OUT_DTYPE.itemsize == 64
    assert replay.EVENT_DTYPE.fields["duration_ns"][1] == 16 and replay.EVENT_DTYPE.fields["status"][1] == 12
    assert replay.EDGE_OUT_DTYPE.fields["from_ref"][1] == 24 and replay.EDGE_OUT_DTYPE.fields["score"][1] == 40
    # every struct and constant the Python side copies, held to the header by the compiler; LAYOUTS must name every twin
    twins = {n: v for n, v in vars(engine).items() if (n.startswith("Sg") and isinstance(v, type) and issubclass(v, C.Structure))
             or (n.endswith("_DTYPE") and isinstance(v, np.dtype))}
    missing = [n for n, v in twins.items() if not any(v is t for t in LAYOUTS.values())]
    assert len(twins) >= 23 and not missing, missing
    src = tmp_path / "layout_check.c"
    src.write_text(layout_check_source())
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


def test_code_object_is_gfx950_only():
    lib = build.build_engine()
    blob = open(lib, "rb").read()
    assert b"gfx950" in blob and b"gfx942" not in blob and b"sm_" not in blob


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="only meaningful without a GPU")
def test_no_cpu_fallback_create_fails_loudly(engine_lib):
    with pytest.raises(engine.ServiceGraphError) as ei:
        engine.ServiceGraph(max_known_nodes=16, max_edges=16)
    assert ei.value.rc == engine.SG_ENODEV


def test_bad_config_rejected(engine_lib):
    cfg = engine.make_config(max_known_nodes=16, max_edges=16)
    h = C.c_void_p()
    cfg.abi_version = 999
    assert engine_lib.sg_create(C.byref(cfg), C.byref(h)) == engine.SG_EINVAL
    cfg.abi_version = engine.ABI_VERSION; cfg.struct_size = 80          # an ABI-2 caller's sg_config: shorter than ABI 3's first layout
    assert engine_lib.sg_create(C.byref(cfg), C.byref(h)) == engine.SG_EINVAL
    cfg.struct_size = 0
    assert engine_lib.sg_create(C.byref(cfg), C.byref(h)) == engine.SG_EINVAL
    assert engine_lib.sg_create(None, C.byref(h)) == engine.SG_EINVAL
    assert engine_lib.sg_destroy(None) == engine.SG_EINVAL


def test_product_never_touches_the_oracle():
    """The oracle is test infrastructure: nothing under alaz_amd/ or include/ may reference it."""
    bad = []
    for base in ("alaz_amd", "include"):
        for dp, _, fs in os.walk(os.path.join(ROOT, base)):
            for f in fs:
                if f.endswith((".py", ".h", ".hpp", ".hip", ".cpp", ".c")):
                    t = open(os.path.join(dp, f), errors="ignore").read()
                    if re.search(r"pyoracle|sg_oracle|libsgoracle|from oracle|import oracle", t):
                        bad.append(os.path.join(dp, f))
    assert not bad, bad


def test_hand_issued_loads_are_never_touched_before_their_wait():
    """tools/check_asm_loads.py on the gfx950 assembly of the engine: no instruction reads or writes a VGPR that
    is the destination of an inline-asm global load before an inline-asm s_waitcnt has covered it (a compiler
    copy there reads stale data; it happened once and only showed up as wrong joins on the GPU)."""
    import subprocess, sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_asm_loads.py")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
