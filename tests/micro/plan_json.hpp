// What the stages of plan_driver.cpp share: the writer of the one JSON object a stage prints per input line, with a plan's memory
// layout (sg_plan.hpp Block) and its per-slot region as members, and the parser of the engine-level stages' `name key=value ...` lines.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <sstream>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../alaz_amd/csrc/sg_plan.hpp"

// One JSON object, written member by member in the order of the calls; objects and arrays nest between obj() / arr() and end().
// A key of nullptr is an element of the array that is open.
class Json {
    std::string s_ = "{";
    std::string close_;                        // the brackets that are open, innermost last
    bool fresh_ = true;                        // nothing yet since the last opening bracket
    void lead(const char* k) {
        if (!fresh_) s_ += ", ";
        fresh_ = false;
        if (k) { s_ += '"'; s_ += k; s_ += "\": "; }
    }
    void open(const char* k, char a, char z) { lead(k); s_ += a; close_ += z; fresh_ = true; }

public:
    template <class T>
    Json& kv(const char* k, T v) {             // a number: floats as the shortest text that parses back to them, bools as 0 / 1
        static_assert(std::is_arithmetic_v<T> || std::is_enum_v<T>, "kv() writes numbers; str() writes strings");
        char b[48];
        if constexpr (std::is_same_v<T, float>) std::snprintf(b, sizeof b, "%g", (double)v);
        else if constexpr (std::is_floating_point_v<T>) std::snprintf(b, sizeof b, "%.17g", (double)v);
        else if constexpr (std::is_signed_v<T>) std::snprintf(b, sizeof b, "%lld", (long long)v);
        else std::snprintf(b, sizeof b, "%llu", (unsigned long long)v);
        lead(k); s_ += b;
        return *this;
    }
    Json& str(const char* k, const std::string& v) {
        lead(k); s_ += '"';
        for (const char ch : v) {
            if (ch == '"' || ch == '\\') { s_ += '\\'; s_ += ch; }
            else if ((unsigned char)ch < 0x20) { char b[8]; std::snprintf(b, sizeof b, "\\u%04x", (unsigned)ch); s_ += b; }
            else s_ += ch;
        }
        s_ += '"';
        return *this;
    }
    Json& null(const char* k = nullptr) { lead(k); s_ += "null"; return *this; }
    Json& obj(const char* k = nullptr) { open(k, '{', '}'); return *this; }
    Json& arr(const char* k = nullptr) { open(k, '[', ']'); return *this; }
    Json& end() { s_ += close_.back(); close_.pop_back(); fresh_ = false; return *this; }
    template <class T>
    Json& list(const char* k, std::initializer_list<T> vs) { arr(k); for (const T v : vs) kv(nullptr, v); return end(); }

    // "<key>": [[name, off, bytes], ...] — the pieces in the order they were taken
    Json& put_layout(const char* key, const std::vector<sgplan::Piece>& l) {
        arr(key);
        for (const sgplan::Piece& p : l) { arr(); str(nullptr, p.name); kv(nullptr, p.off); kv(nullptr, p.bytes); end(); }
        return end();
    }
    // "slot": [off, bytes], "slot_rel": {name: offset inside a slot, ...} — the per-slot region as servicegraph.hip reads it
    Json& put_slot(const sgplan::Slots& s, std::initializer_list<std::pair<const char*, sgplan::u64>> rel) {
        list("slot", {s.off, s.bytes});
        obj("slot_rel");
        for (const auto& r : rel) kv(r.first, r.second);
        return end();
    }
    void emit() { std::printf("%s}\n", s_.c_str()); }      // (every bracket but the object's own is closed by now)
};
// a member whose JSON key is its own name, into the writer `j` of the stage
#define PUT(s, m) j.kv(#m, (s).m)

// One line `name key=value ...` of an engine-level stage: sg_config members by name, every knob of kKnobs (as SG_* names them) and
// cus= (the compute units of `dev`, which the caller owns).  Keys it does not know come back in `rest` for the stage to take or refuse.
struct Case {
    std::string name;
    sg_config c;
    sgplan::Overrides ov;
    std::vector<std::pair<std::string, sgplan::u64>> rest;
};

inline Case parse_case(const std::string& line, sgplan::DeviceFacts& dev) {
    Case cs;
    sg_config& c = cs.c;
    std::memset(&c, 0, sizeof c);
    c.struct_size = sizeof c; c.abi_version = SG_ABI_VERSION; c.layers = 2; c.world = 1; c.max_outbound_ips = 64; c.max_labels = 64;
    std::istringstream is(line);
    std::string tok;
    is >> cs.name;
    while (is >> tok) {
        const size_t eq = tok.find('=');
        const std::string k = tok.substr(0, eq), v = tok.substr(eq + 1);
        const sgplan::u64 x = std::strtoull(v.c_str(), nullptr, 0);
        bool known = false;
        for (const sgplan::KnobName& kn : sgplan::kKnobs) if (k == kn.name) { cs.ov.*kn.field = v; known = true; }
#define CFG(m) if (k == #m) { c.m = (decltype(c.m))x; known = true; }
        CFG(max_known_nodes) CFG(max_labels) CFG(max_outbound_ips) CFG(max_ips) CFG(max_edges) CFG(max_batch) CFG(layers) CFG(rank)
        CFG(world) CFG(k1_variant) CFG(max_window_events) CFG(windows_in_flight) CFG(max_alive) CFG(flags)
#undef CFG
        if (k == "cus") { dev.cus = (int)x; known = true; }
        if (!known) cs.rest.emplace_back(k, x);
    }
    return cs;
}
