// heatray_amd/csrc/hr_tune.h on the CPU (tests/test_tune_parse.py builds this with -fsanitize=address,undefined and runs it): the
// defaults, the table and the parser of the HR_TUNE string.  No input; prints "tune parse cpu: ok" and returns 0 when every check holds.
#include "hr_tune.h"

#include <cstdio>

static int failures = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) printf("line %d: %s\n", __LINE__, #cond), ++failures; \
    } while (0)

static bool sameKnobs(const Tune &a, const Tune &b)
{
    for (const TuneKnob &k : kTuneKnobs)
        if (a.*k.member != b.*k.member) return false;
    return a.blocksSet == b.blocksSet && a.debugPipe == b.debugPipe && a.debugStepTimes == b.debugStepTimes;
}

// `text` fails and the message names `item`
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
    // the defaults: the fields of hr_ctx before the table existed (kMaxSlots = 2 * HR_MAX_SEGS = 640 passes in flight)
    const struct {
        const char *key;
        int value;
    } defaults[] = {{"tri", 2},     {"refill", 16}, {"blocks", 5},  {"sblocks", 4}, {"depth", 640}, {"batch", 0},  {"fmax", 64},   {"fmin", 64},
                    {"groups", 0},  {"prio", 1},    {"refit", 1},   {"sdeal", 256}, {"guard", 125}, {"ploc", 1},   {"plocr", 16},  {"packets", 2},
                    {"corun", 1},   {"cmin", 50},   {"cblocks", 0}, {"plog", -1},   {"pswz", 1},    {"pstep", 1},  {"pstepf", 110}, {"pprobe", 0},
                    {"punion", 220}, {"fprim", 128}, {"fgate", 8},  {"heads", 5},   {"slow", 4},    {"ovf", 0}};
    const Tune fresh;
    CHECK(sizeof(defaults) / sizeof(defaults[0]) == kTuneKnobCount && kTuneKnobCount == 30);
    for (size_t i = 0; i < kTuneKnobCount && i < sizeof(defaults) / sizeof(defaults[0]); ++i) {
        CHECK(strcmp(kTuneKnobs[i].key, defaults[i].key) == 0);
        if (fresh.*kTuneKnobs[i].member != defaults[i].value) printf("default of %s: %d\n", kTuneKnobs[i].key, fresh.*kTuneKnobs[i].member), ++failures;
        CHECK(kTuneKnobs[i].lo <= defaults[i].value && defaults[i].value <= kTuneKnobs[i].hi && kTuneKnobs[i].doc && kTuneKnobs[i].doc[0]);
        for (size_t j = 0; j < i; ++j) CHECK(strcmp(kTuneKnobs[i].key, kTuneKnobs[j].key) != 0 && kTuneKnobs[i].member != kTuneKnobs[j].member);
    }
    CHECK(!fresh.blocksSet && !fresh.debugPipe && !fresh.debugStepTimes);
    CHECK(kMaxSlots == 640 && kMaxGroups == 3);

    // nothing to parse: an empty string (tools set HR_TUNE=""), commas alone
    for (const char *text : {"", ",", ",,,"}) {
        Tune t;
        CHECK(parseTune(text, t, err) && sameKnobs(t, fresh));
    }

    // every key round-trips with a value inside its range, alone and with empty items around it, and touches nothing else
    for (const TuneKnob &k : kTuneKnobs) {
        for (const int value : {k.lo, k.hi, k.lo > 3 ? k.lo : (k.hi < 3 ? k.hi : 3)}) {
            for (const char *form : {"%s=%d", ",%s=%d,", "%s=%d,,"}) {
                char text[64];
                snprintf(text, sizeof(text), form, k.key, value);
                Tune t, want;
                want.*k.member = value, want.blocksSet = k.member == &Tune::blocks;
                if (!parseTune(text, t, err) || !sameKnobs(t, want)) printf("round trip of '%s': %s\n", text, err.c_str()), ++failures;
            }
        }
    }
    {
        Tune t;
        CHECK(parseTune("plog=+3,cmin=-7,guard=0042", t, err) && t.plog == 3 && t.cmin == -7 && t.guard == 42);
    }

    // blocks= is remembered as given; the keys that end in "blocks" are their own
    {
        Tune a, b, c;
        CHECK(parseTune("blocks=4", a, err) && a.blocksSet && a.blocks == 4);
        CHECK(parseTune("sblocks=4", b, err) && !b.blocksSet && b.blocks == 5 && b.sblocks == 4);
        CHECK(parseTune("cblocks=4", c, err) && !c.blocksSet && c.blocks == 5 && c.cblocks == 4);
    }

    // a repeated key keeps its first value (bench.py appends ",batch=1" to the caller's string)
    {
        Tune t;
        CHECK(parseTune("batch=3,batch=1", t, err) && t.batch == 3);
        Tune u;
        CHECK(parseTune("packets=0,batch=3,packets=1,batch=1", u, err) && u.batch == 3 && u.packets == 0);
    }

    // errors name the item
    fails("leaf=4", "leaf=4");
    fails("packets=1,leaf=4", "leaf=4");
    fails("leaf=4,tri=20", "leaf=4");
    fails("packets", "packets");
    fails("packets=", "packets=");
    fails("packets=x", "packets=x");
    fails("packets=1x", "packets=1x");
    fails("packets= 1", "packets= 1");
    fails("packets=-", "packets=-");
    fails("packets=1,=3", "=3");
    fails("batch=99999999999999999999", "batch=99999999999999999999");
    fails("batch=4294967297", "batch=4294967297");
    fails("groups=4", "groups=4");
    fails("groups=-1", "groups=-1");
    fails("groups=4,batch=16", "groups=4");
    fails("depth=0", "depth=0");
    fails("depth=641", "depth=641");
    fails("heads=7", "heads=7");
    fails("heads=-1", "heads=-1");
    fails("fmax=0", "fmax=0");
    fails("fmin=0", "fmin=0");
    fails("fprim=0", "fprim=0");
    fails("tblk=0", "tblk=0");
    fails("sprobe=1", "sprobe=1");
    fails("Packets=1", "Packets=1");
    fails("batch=3,batch=x", "batch=x"); // (a repeat is skipped only once it is well-formed)

    // every string the suite sets HR_TUNE to (tests/test_gpu_*.py, tests/test_hit_rule.py), and the tools' (bench.py's repeat included)
    const char *inUse[] = {"", "packets=0", "packets=1", "packets=2", "batch=1", "batch=5,groups=2", "ploc=0", "ploc=1", "ploc=2", "ploc=2,plocr=3",
                           "packets=1,corun=0", "packets=1,corun=2", "packets=1,corun=2,cblocks=1", "packets=1,pstep=1", "packets=1,pstep=0",
                           "pprobe=0", "pprobe=1", "packets=2,punion=1000,pstepf=150", "packets=2,punion=1000,pstepf=100", "packets=2,punion=101",
                           "punion=115", "packets=1,batch=5", "packets=1,batch=2", "groups=1,batch=1", "groups=2", "groups=3,batch=2",
                           "groups=2,batch=5,depth=24", "fmin=16,fmax=256,refill=16,tri=8,blocks=3", "batch=16", "sdeal=0,batch=3",
                           "sdeal=1000000,groups=1", "sdeal=0,heads=0,fprim=256,fgate=0", "sdeal=0,heads=6,fprim=32,fgate=0,fmin=16,batch=7",
                           "batch=1,slow=0", "slow=0", "groups=2,batch=1", "ovf=1,packets=0", "ovf=2,packets=0", "ovf=3,packets=0",
                           "ovf=1,packets=1", "ovf=2,packets=1", "ovf=3,packets=1", "packets=1,", "guard=100000", "plog=4", "groups=2,blocks=5",
                           "packets=1,corun=2,batch=1", "batch=12,batch=1"};
    for (const char *text : inUse) {
        Tune t;
        if (!parseTune(text, t, err)) printf("'%s' must parse: %s\n", text, err.c_str()), ++failures;
    }
    {
        Tune t;
        CHECK(parseTune("sdeal=0,heads=6,fprim=32,fgate=0,fmin=16,batch=7", t, err) && t.sdeal == 0 && t.heads == 6 && t.fprim == 32 && t.fgate == 0 && t.fmin == 16 &&
              t.batch == 7 && t.fmax == 64);
    }
    if (failures) return printf("tune parse cpu: %d checks failed\n", failures), 1;
    printf("tune parse cpu: ok\n");
    return 0;
}
