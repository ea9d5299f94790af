// Tuning knobs as table rows (host only).  A knob's value lives in a named
// std::atomic<int> that the code reading it loads directly; a row ties that
// storage to the knob's name, its accepted values and -- for a kernel knob --
// the kern::Variant member it overrides, and the set / get / override / describe
// paths are loops over the rows (ec_core.cpp and submit.cpp hold the tables).
// Nothing on a per-call path looks a knob up by name.
#pragma once

#include <atomic>
#include <climits>
#include <cstddef>
#include <cstdio>
#include <cstring>

namespace shmr {
namespace knobs {

constexpr int kAuto = -2;      // "reset": the row says what it resolves to
constexpr int kOk = 0;         // SHMR_EC_OK
constexpr int kInvalid = -100; // SHMR_EC_INVALID_ARGUMENT
#ifdef SHMR_EC_TOOLS
constexpr bool kToolsBuild = true;
#else
constexpr bool kToolsBuild = false;
#endif

// The values a knob takes besides kAuto: a range, or a short list (n > 0).
struct Accept {
    int lo, hi;
    int n;
    int list[6];
    constexpr bool has(int v) const {
        if (n == 0) return v >= lo && v <= hi;
        for (int i = 0; i < n; ++i)
            if (list[i] == v) return true;
        return false;
    }
};
constexpr Accept range(int lo, int hi) { return Accept{lo, hi, 0, {}}; }
constexpr Accept any() { return range(INT_MIN, INT_MAX); }
template <class... I>
constexpr Accept among(I... v) {
    static_assert(sizeof...(v) >= 1 && sizeof...(v) <= 6, "a short list");
    return Accept{0, -1, int(sizeof...(v)), {v...}};
}

enum Scope {
    kExact,     // one value for the process; the key is the bare name
    kProcess,   // one value for the process; an "encode." / "decode." prefix is accepted and ignored
    kPerClass,  // one value per op class; a bare key sets both and reads the encode one
};
enum Use {
    kStored,    // read from its storage where it applies
    kOverride,  // a value other than kAuto replaces the variant member
    kOnlyOff,   // only 0 replaces the variant member (with false)
};

template <class V>
struct Knob {
    const char* name;
    Scope scope;
    std::atomic<int>* at[2];   // [encode], [decode]; a process-wide knob names its one atomic twice
    int dflt;                  // the value it starts with, and what kAuto resolves to
    bool auto_ok;              // false: kAuto is a value like any other
    Accept tools, product;     // accepted besides kAuto, per flavour of the library
    bool to_bool;              // a non-zero value is stored as 1
    // kernel knobs: the variant member (one of the two), how the knob acts on
    // it, and whether " name=1" is appended to the describe string when it is set
    Use use;
    int V::*vi;
    bool V::*vb;
    bool tail;
};

// A knob of the tools build: the product build takes only its default.
template <class V>
constexpr Knob<V> tools_only(Knob<V> k) {
    k.product = among(k.dflt);
    return k;
}

namespace detail {
// The key's row; [*first, *last] are the op classes its prefix names.
template <class V, size_t N>
const Knob<V>* find(const Knob<V> (&table)[N], const char* key, int* first, int* last) {
    if (!key) return nullptr;
    const bool enc = std::strncmp(key, "encode.", 7) == 0, dec = std::strncmp(key, "decode.", 7) == 0;
    *first = dec ? 1 : 0;
    *last = enc ? 0 : 1;
    const char* name = key + (enc || dec ? 7 : 0);
    for (const Knob<V>& k : table)
        if (std::strcmp(k.name, k.scope == kExact ? key : name) == 0) return &k;
    return nullptr;
}
}  // namespace detail

// Sets knob `key`; *known = false (and kInvalid) when the table has no such knob.
template <class V, size_t N>
int knob_set(const Knob<V> (&table)[N], const char* key, int value, bool* known) {
    int first = 0, last = 1;
    const Knob<V>* k = detail::find(table, key, &first, &last);
    *known = k != nullptr;
    if (!k) return kInvalid;
    int v = value;
    if (k->auto_ok && value == kAuto) {
        v = k->dflt;
    } else {
        if (!(kToolsBuild ? k->tools : k->product).has(value)) return kInvalid;
        if (k->to_bool) v = value != 0;
    }
    for (int i = first; i <= last; ++i) k->at[i]->store(v);
    return kOk;
}

// The knob's value (of the encode class for a bare per-class key); kInvalid
// and *known = false when the table has no such knob.
template <class V, size_t N>
int knob_get(const Knob<V> (&table)[N], const char* key, bool* known) {
    int first = 0, last = 1;
    const Knob<V>* k = detail::find(table, key, &first, &last);
    *known = k != nullptr;
    return k ? k->at[first]->load() : kInvalid;
}

// The kernel knobs of op class `op` applied to a policy variant.
template <class V, size_t N>
void knob_override(const Knob<V> (&table)[N], int op, V* v) {
    for (const Knob<V>& k : table) {
        if (k.use == kStored) continue;
        const int x = k.at[op]->load();
        if (k.use == kOnlyOff ? x != 0 : x == kAuto) continue;
        if (k.vi) v->*k.vi = x;
        if (k.vb) v->*k.vb = x != 0;
    }
}

// Appends " name=1" for every set member of the table's `tail` rows, in table order.
template <class V, size_t N>
void knob_describe_tail(const Knob<V> (&table)[N], const V& v, char* buf, size_t len) {
    for (const Knob<V>& k : table) {
        const size_t n = std::strlen(buf);
        if (k.tail && v.*k.vb && n + 1 < len) std::snprintf(buf + n, len - n, " %s=1", k.name);
    }
}

}  // namespace knobs
}  // namespace shmr
