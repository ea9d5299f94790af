// CPU check of the knob table code (shmr_amd/csrc/knobs.hpp) for
// tests/test_knobs.py: a table with one knob of each kind, driven through
// knob_set / knob_get with every key form and value against a model written
// out below, then knob_override and knob_describe_tail.  Built with and without
// -DSHMR_EC_TOOLS; prints "ok <checks>" or the first mismatch (exit status 1).
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "knobs.hpp"

namespace kn = shmr::knobs;

struct V {
    int u = 1;
    bool early = false, occ8 = false, fuse = true, glds = false;
};
using K = kn::Knob<V>;

std::atomic<int> g_flag[2], g_occ8[2], g_u[2], g_fuse[2], g_glds[2], g_spin, g_uvec, g_alias, g_lead, g_on;

enum { kFlag, kOcc8, kU, kFuse, kGlds, kSpin, kUvec, kAlias, kLead, kOn, kKnobs };
const K kTable[] = {
    kn::tools_only(K{"early", kn::kPerClass, {&g_flag[0], &g_flag[1]}, kn::kAuto, true, kn::any(), kn::any(), true,
                     kn::kOverride, nullptr, &V::early, false}),
    kn::tools_only(K{"occ8", kn::kPerClass, {&g_occ8[0], &g_occ8[1]}, 0, false, kn::any(), kn::any(), true,
                     kn::kOverride, nullptr, &V::occ8, false}),
    kn::tools_only(K{"chunks", kn::kPerClass, {&g_u[0], &g_u[1]}, kn::kAuto, true, kn::among(1, 2, 4), kn::any(),
                     false, kn::kOverride, &V::u, nullptr, false}),
    kn::tools_only(K{"fuse", kn::kPerClass, {&g_fuse[0], &g_fuse[1]}, kn::kAuto, true, kn::any(), kn::any(), true,
                     kn::kOnlyOff, nullptr, &V::fuse, false}),
    kn::tools_only(K{"glds", kn::kPerClass, {&g_glds[0], &g_glds[1]}, kn::kAuto, true, kn::any(), kn::any(), true,
                     kn::kStored, nullptr, &V::glds, true}),
    K{"spin_us", kn::kProcess, {&g_spin, &g_spin}, 7, true, kn::range(0, INT_MAX), kn::range(0, INT_MAX), false,
      kn::kStored, nullptr, nullptr, false},
    K{"uvec", kn::kProcess, {&g_uvec, &g_uvec}, kn::kAuto, true, kn::among(0, 1), kn::among(0), false, kn::kStored,
      nullptr, nullptr, false},
    kn::tools_only(K{"alias", kn::kProcess, {&g_alias, &g_alias}, 0, true, kn::range(0, 32), kn::any(), false,
                     kn::kStored, nullptr, nullptr, false}),
    K{"lead_us", kn::kExact, {&g_lead, &g_lead}, 30, true, kn::range(0, 10000000), kn::range(0, 10000000), false,
      kn::kStored, nullptr, nullptr, false},
    K{"on", kn::kExact, {&g_on, &g_on}, 1, true, kn::range(0, 1), kn::range(0, 1), false, kn::kStored, nullptr,
      nullptr, false},
};
const int kDefault[kKnobs] = {-2, 0, -2, -2, -2, 7, -2, 0, 30, 1};

// The model: whether knob `i` takes `v`, and what it then holds.
bool model(int i, int v, int* stored) {
    const bool tools = kn::kToolsBuild;
    *stored = v;
    switch (i) {
        case kFlag: case kFuse: case kGlds:
            if (v == -2) return true;
            *stored = v != 0;
            return tools;
        case kOcc8:
            *stored = v != 0;   // -2 is no reset here: it stores 1
            return tools || v == 0;
        case kU: return v == -2 || (tools && (v == 1 || v == 2 || v == 4));
        case kSpin:
            if (v == -2) *stored = 7;
            return v == -2 || v >= 0;
        case kUvec: return v == -2 || v == 0 || (tools && v == 1);
        case kAlias:
            if (v == -2) *stored = 0;
            return v == -2 || v == 0 || (tools && v > 0 && v <= 32);
        case kLead:
            if (v == -2) *stored = 30;
            return v == -2 || (v >= 0 && v <= 10000000);
        default:
            if (v == -2) *stored = 1;
            return v == -2 || v == 0 || v == 1;
    }
}

long g_checks = 0;
#define CHECK(cond, ...)                          \
    do {                                          \
        ++g_checks;                               \
        if (!(cond)) {                            \
            std::printf("FAILED " __VA_ARGS__);   \
            std::printf(" (%s)\n", #cond);        \
            std::exit(1);                         \
        }                                         \
    } while (0)

int main() {
    const int values[] = {-3, -2, -1, 0, 1, 2, 3, 4, 5, 6, 7, 9, 32, 33, 64, 128, 256, 512, 65536, 65537, 10000001,
                          INT_MIN, INT_MAX};
    const char* prefixes[] = {"", "encode.", "decode."};
    int shadow[kKnobs][2];
    for (int i = 0; i < kKnobs; ++i) {
        shadow[i][0] = shadow[i][1] = kDefault[i];
        kTable[i].at[0]->store(kDefault[i]);
        kTable[i].at[1]->store(kDefault[i]);
    }
    bool known = false;
    for (int i = 0; i < kKnobs; ++i)
        for (int p = 0; p < 3; ++p)
            for (int v : values) {
                const std::string key = std::string(prefixes[p]) + kTable[i].name;
                const bool exact = kTable[i].scope == kn::kExact;
                const bool per_class = kTable[i].scope == kn::kPerClass;
                const int rc = kn::knob_set(kTable, key.c_str(), v, &known);
                if (exact && p) {   // a prefixed key names no knob of this kind
                    CHECK(rc == kn::kInvalid && !known, "%s=%d", key.c_str(), v);
                } else {
                    int stored = 0;
                    const bool ok = model(i, v, &stored);
                    CHECK(known && rc == (ok ? kn::kOk : kn::kInvalid), "%s=%d -> %d", key.c_str(), v, rc);
                    for (int c = 0; ok && c < 2; ++c)
                        if (!per_class || p == 0 || p == c + 1) shadow[i][c] = stored;
                }
                for (int j = 0; j < kKnobs; ++j)   // every knob reads back what the model holds
                    for (int q = 0; q < 3; ++q) {
                        const std::string k2 = std::string(prefixes[q]) + kTable[j].name;
                        const int got = kn::knob_get(kTable, k2.c_str(), &known);
                        if (kTable[j].scope == kn::kExact && q)
                            CHECK(got == kn::kInvalid && !known, "get %s", k2.c_str());
                        else
                            CHECK(known && got == shadow[j][q == 2], "get %s = %d after %s=%d", k2.c_str(), got,
                                  key.c_str(), v);
                    }
            }
    // keys that name nothing; none may change a value
    const std::string longkey(200000, 'x');
    const std::string keys[] = {"", "encode.", "decode.", "encode", ".", "earl", "early ", "earlyx", "Early",
                                "encode.encode.early", "decode.encode.early", "encode.decode.chunks", "encode.on",
                                "decode.lead_us", "lead_us.", longkey, "encode." + longkey, "early" + longkey};
    for (const std::string& k : keys) {
        CHECK(kn::knob_set(kTable, k.c_str(), 1, &known) == kn::kInvalid && !known, "set '%.20s'", k.c_str());
        CHECK(kn::knob_get(kTable, k.c_str(), &known) == kn::kInvalid && !known, "get '%.20s'", k.c_str());
    }
    known = true;
    CHECK(kn::knob_set(kTable, nullptr, 1, &known) == kn::kInvalid && !known, "set null");
    known = true;
    CHECK(kn::knob_get(kTable, nullptr, &known) == kn::kInvalid && !known, "get null");
    for (int i = 0; i < kKnobs; ++i)
        for (int c = 0; c < 2; ++c) CHECK(kTable[i].at[c]->load() == shadow[i][c], "knob %d changed", i);

    // overrides: per class, kAuto leaves the policy's value, kOnlyOff acts on 0 alone, kStored never
    for (int i = 0; i < kKnobs; ++i) {
        kTable[i].at[0]->store(kDefault[i]);
        kTable[i].at[1]->store(kDefault[i]);
    }
    g_u[1] = 4;
    g_flag[1] = 1;
    g_occ8[1] = 1;
    g_fuse[0] = 1;
    g_fuse[1] = 0;
    g_glds[0] = g_glds[1] = 1;
    V enc, dec;
    enc.fuse = false;
    kn::knob_override(kTable, 0, &enc);
    kn::knob_override(kTable, 1, &dec);
    CHECK(enc.u == 1 && !enc.early && !enc.occ8 && !enc.fuse && !enc.glds, "encode overrides");
    CHECK(dec.u == 4 && dec.early && dec.occ8 && !dec.fuse && !dec.glds, "decode overrides");

    // the describe tail: appended to what the buffer holds, never past its end
    dec.glds = true;
    for (size_t len = 1; len <= 24; ++len) {
        std::vector<char> buf(len);   // (exactly len bytes: a write past it is a sanitizer report)
        std::snprintf(buf.data(), len, "head=1");
        const std::string head = buf.data();
        kn::knob_describe_tail(kTable, enc, buf.data(), len);
        CHECK(head == buf.data(), "tail of an unset member, len %zu", len);
        kn::knob_describe_tail(kTable, dec, buf.data(), len);
        const std::string want = head.size() + 1 < len ? (head + " glds=1").substr(0, len - 1) : head;
        CHECK(want == buf.data(), "tail '%s' at len %zu", buf.data(), len);
    }
    std::printf("ok %ld\n", g_checks);
    return 0;
}
