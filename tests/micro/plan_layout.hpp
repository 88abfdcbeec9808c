// What the stage plans' CPU drivers share: a plan's memory layout (sg_plan.hpp Block) as JSON members of the object a driver prints.
#pragma once
#include <cstdio>
#include <initializer_list>
#include <utility>
#include <vector>

#include "../../alaz_amd/csrc/sg_plan.hpp"

// , "<key>": [[name, off, bytes], ...] — the pieces in the order they were taken
inline void put_layout(const char* key, const std::vector<sgplan::Piece>& l) {
    std::printf(", \"%s\": [", key);
    for (size_t i = 0; i < l.size(); i++)
        std::printf("%s[\"%s\", %llu, %llu]", i ? ", " : "", l[i].name, (unsigned long long)l[i].off, (unsigned long long)l[i].bytes);
    std::printf("]");
}
// , "slot": [off, bytes], "slot_rel": {name: offset inside a slot, ...} — the per-slot region as servicegraph.hip reads it
inline void put_slot(const sgplan::Slots& s, std::initializer_list<std::pair<const char*, sgplan::u64>> rel) {
    std::printf(", \"slot\": [%llu, %llu], \"slot_rel\": {", (unsigned long long)s.off, (unsigned long long)s.bytes);
    const char* sep = "";
    for (const auto& r : rel) { std::printf("%s\"%s\": %llu", sep, r.first, (unsigned long long)r.second); sep = ", "; }
    std::printf("}");
}
