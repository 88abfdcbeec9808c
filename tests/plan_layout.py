"""What the CPU tests of the opt-in stages' plans share: the checks of a stage block's memory layout as its driver under tests/micro
prints it (tests/micro/plan_json.hpp) — "layout": [[name, off, bytes], ...] in the order sg_plan.hpp's Block handed the pieces
out, "slot": [off, bytes] and "slot_rel": {name: offset inside a slot} for the per-slot region.  servicegraph.hip adds exactly these
offsets to the block's base, so a piece that overlaps its neighbour, runs past total_bytes or is smaller than what a kernel writes
fails here, on the CPU."""
from collections import Counter

SOA = ("from_key", "to_key", "lat_mean", "lat_dev", "err_mean", "err_dev", "n", "last")


def check_layout(r, need, per_slot=(), align=256, layout="layout", total="total_bytes", slots=None, tail_align=None):
    """r: one object of a plan driver.  need: {piece name: the bytes it must hold at least} — every piece of the layout is named in
    it.  per_slot: the pieces every window slot has.  tail_align: the size of the LAST piece is a multiple of this instead of align
    (K7's u32 keys end its scratch: scratch_bytes is their end, not rounded)."""
    lay = r[layout]
    slots = max(r["slots"], 1) if slots is None else slots
    assert lay[0][1] == 0, lay[0]                                        # the first piece is at 0
    for (_, o0, b0), (n1, o1, _) in zip(lay, lay[1:]):
        assert o1 == o0 + b0, (n1, o1, o0 + b0)                          # each piece begins where the previous one ends
    for i, (n, o, b) in enumerate(lay):
        assert o % align == 0, (n, o)
        assert b % (tail_align if tail_align and i == len(lay) - 1 else align) == 0, (n, b)
    assert lay[-1][1] + lay[-1][2] == r[total]                           # the last piece ends at total_bytes
    times = Counter(n for n, _, _ in lay)
    assert set(times) == set(need), (sorted(times), sorted(need))
    for n, c in times.items():
        assert c == (slots if n in per_slot else 1), (n, c)              # every per-slot piece exactly `slots` times
    for n, _, b in lay:
        assert b >= need[n], (n, b, need[n])
    if not per_slot:
        return
    off, stride = r["slot"]
    assert set(r["slot_rel"]) == set(per_slot) and off + slots * stride == r[total]   # the per-slot region is the block's tail
    assert off % align == 0 and stride % align == 0
    for n in per_slot:
        at = [o for m, o, _ in lay if m == n]
        assert len({b - a for a, b in zip(at, at[1:])}) <= 1             # a constant stride
        assert at == [off + k * stride + r["slot_rel"][n] for k in range(slots)], n   # ... the one servicegraph.hip steps by
    shared = [o + b for m, o, b in lay if m not in per_slot]
    assert max(shared, default=0) <= off                                 # no shared piece inside the per-slot region


def check_soa(r):
    """the eight arrays of one baseline buffer ("soa_layout", entries = max_entries): back to back from 0 in TrendSoA's order, each
    holding its entries, the 64-bit arrays 8-byte aligned, and the last one ending within soa_bytes.

    `last`, the second u32 array, begins where `n` ends — at 52 x entries, which an odd max_entries leaves 4-byte and not 8-byte
    aligned (max_entries 1: 52).  Back to back and 8-byte aligned cannot both hold there; the kernels read u32 words, and the
    addresses stay what they were, so `last` is held to the alignment of its elements (and to 8 bytes whenever max_entries is even)."""
    lay, C = r["soa_layout"], r["entries"]
    assert tuple(n for n, _, _ in lay) == SOA
    assert lay[0][1] == 0
    for (_, o0, b0), (n1, o1, _) in zip(lay, lay[1:]):
        assert o1 == o0 + b0, (n1, o1, o0 + b0)
    for n, o, b in lay:
        wide = n not in ("n", "last")
        assert b == C * (8 if wide else 4), (n, b)
        assert o % (8 if wide or n == "n" or C % 2 == 0 else 4) == 0, (n, o)
    assert lay[-1][1] + lay[-1][2] <= r["soa_bytes"]
