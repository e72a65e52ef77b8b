// heatray_amd/csrc/hr_tune.h on the CPU (tests/test_sah_subtree.py builds this with -fsanitize=address,undefined and runs it): the knobs
// of the second table, kTuneBuildKnobs (sahsub), go through the same parser with the same rules as those of kTuneKnobs, which
// tests/host/tune_parse_cpu.cpp holds.  No input; prints "tune build knobs cpu: ok" and returns 0 when every check holds.
#include "hr_tune.h"

#include <cstdio>

static int failures = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) printf("line %d: %s\n", __LINE__, #cond), ++failures; \
    } while (0)

static void fails(const char *text, const char *item)
{
    Tune t;
    std::string err;
    const bool ok = parseTune(text, t, err);
    if (ok || err.find(item) == std::string::npos) printf("'%s' must fail naming '%s': %s, \"%s\"\n", text, item, ok ? "parsed" : "failed", err.c_str()), ++failures;
}

int main()
{
    std::string err;
    const Tune fresh;
    CHECK(kTuneBuildKnobCount == 1 && strcmp(kTuneBuildKnobs[0].key, "sahsub") == 0 && fresh.sahsub == 64);
    for (const TuneKnob &b : kTuneBuildKnobs) {
        CHECK(b.doc && b.doc[0] && b.lo <= fresh.*b.member && fresh.*b.member <= b.hi);
        for (const TuneKnob &k : kTuneKnobs) CHECK(strcmp(k.key, b.key) != 0 && k.member != b.member); // no key and no field twice
        for (const int value : {b.lo, b.hi, 3})
            for (const char *form : {"%s=%d", ",%s=%d,", "packets=1,%s=%d", "%s=%d,batch=3"}) {
                char text[64];
                snprintf(text, sizeof(text), form, b.key, value);
                Tune t;
                CHECK(parseTune(text, t, err) && t.*b.member == value);
                Tune rest = t; // ... and touches nothing else but what the string names
                rest.*b.member = fresh.*b.member, rest.packets = fresh.packets, rest.batch = fresh.batch;
                for (const TuneKnob &k : kTuneKnobs) CHECK(rest.*k.member == fresh.*k.member);
                CHECK(!t.blocksSet);
            }
    }
    {
        Tune t;
        CHECK(parseTune("sahsub=0,sahsub=64", t, err) && t.sahsub == 0); // a repeated key keeps its first value
        Tune u;
        CHECK(parseTune("ploc=0,sahsub=+17,plocr=3", u, err) && u.sahsub == 17 && u.ploc == 0 && u.plocr == 3);
    }
    fails("sahsub=65", "sahsub=65");
    fails("sahsub=-1", "sahsub=-1");
    fails("sahsub=", "sahsub=");
    fails("sahsub", "sahsub");
    fails("sahsub=x", "sahsub=x");
    fails("sahsubs=3", "sahsubs=3");
    fails("sahsu=3", "sahsu=3");
    fails("sahsub=64,leaf=4", "leaf=4");
    // every string the tests of the rebuild set
    for (const char *text : {"sahsub=0", "sahsub=64", "sahsub=64,packets=1", "sahsub=0,packets=1"}) {
        Tune t;
        if (!parseTune(text, t, err)) printf("'%s' must parse: %s\n", text, err.c_str()), ++failures;
    }
    if (failures) return printf("tune build knobs cpu: %d checks failed\n", failures), 1;
    printf("tune build knobs cpu: ok\n");
    return 0;
}
