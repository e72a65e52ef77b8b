// hr_tune.h — the HR_TUNE knobs: one struct of integers, ONE table that names, bounds and documents each of them (and a second, kTuneBuildKnobs, for the tree builder's later ones), and the parser of the
// comma-separated key=value string hr_ctx_create reads from the environment.  Host-only C++ without a HIP include, so that
// tests/host/tune_parse_cpu.cpp checks it without a device.  The defaults were measured on MI355X; the knobs exist for experiments
// (every A/B in profiles/) and for the tests that force a code path (packets=0|1, ploc=0|2, ovf=1..3, slow=0, ...).
#pragma once
#include <cerrno>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <string>

#ifndef HR_MAX_SEGS
#define HR_MAX_SEGS 320 // entries of a step table (hr_kernels.h, which has the same default; hr_ctx.h asserts that the two agree)
#endif
static const int kMaxGroups = 3;
static const int kMaxSlots = 2 * HR_MAX_SEGS; // passes in flight over all groups

struct Tune {
    int tri = 2, refill = 16, blocks = 5, sblocks = 4, depth = kMaxSlots, batch = 0, fmax = 64, fmin = 64;
    int groups = 0, prio = 1, refit = 1, sdeal = 256, guard = 125, ploc = 1, plocr = 16;
    int packets = 2, corun = 1, cmin = 50, cblocks = 0, plog = -1, pswz = 1, pstep = 1, pstepf = 110, pprobe = 0, punion = 220;
    int fprim = 128, fgate = 8, heads = 5, slow = 4, ovf = 0, sahsub = 64;
    bool blocksSet = false; // blocks= was given: hr_frame_resize then leaves k_trace's workgroups per CU at it (hr_ctx::traceBlocks)
    bool debugPipe = false, debugStepTimes = false; // not knobs: HR_DEBUG_PIPE / HR_DEBUG_STEPTIMES are set in the environment (hr_ctx_create reads them once, beside HR_TUNE)
};

// one row per knob; a value outside lo..hi is an error (only where the code relies on the range: every other knob takes any int)
struct TuneKnob { const char *key; int Tune::*member; int lo, hi; const char *doc; };

static const TuneKnob kTuneKnobs[] = {
    {"tri", &Tune::tri, INT_MIN, INT_MAX, "k_trace runs the triangle phase once this many lanes are blocked on a postponed leaf"},
    {"refill", &Tune::refill, INT_MIN, INT_MAX, "k_trace refills a wave from the work pool once this many lanes are idle"},
    {"blocks", &Tune::blocks, INT_MIN, INT_MAX, "k_trace's workgroups per CU (not given: 5 with one pipeline group, 3 with several)"},
    {"sblocks", &Tune::sblocks, INT_MIN, INT_MAX, "the shading kernels' workgroups per CU"},
    {"depth", &Tune::depth, 1, kMaxSlots, "passes in flight, all groups"},
    {"batch", &Tune::batch, INT_MIN, INT_MAX, "passes injected per macro step (0: by the frame's size, hr_frame_resize)"},
    {"fmax", &Tune::fmax, 1, INT_MAX, "work items a wave reserves per global atomic while plenty of work is left ..."},
    {"fmin", &Tune::fmin, 1, INT_MAX, "... shrinking to this near the end of the pool"},
    {"groups", &Tune::groups, 0, kMaxGroups, "pipeline groups (0 = automatic)"},
    {"prio", &Tune::prio, INT_MIN, INT_MAX, "prio=0: worker streams at normal priority"},
    {"refit", &Tune::refit, INT_MIN, INT_MAX, "refit=0: always rebuild"},
    {"sdeal", &Tune::sdeal, INT_MIN, INT_MAX, "launches of at most this many rays per resident wave are dealt out statically (k_trace)"},
    {"guard", &Tune::guard, INT_MIN, INT_MAX, "a refit whose boxes' area exceeds N % of the built tree's rebuilds instead (profiles/r3j_instanced_refit.txt)"},
    {"ploc", &Tune::ploc, INT_MIN, INT_MAX, "ploc=0|1|2: tree builder (hr_build.hip: buildLBVH keeps the cheaper of the radix tree and PLOC)"},
    {"plocr", &Tune::plocr, INT_MIN, INT_MAX, "PLOC's search radius"},
    {"packets", &Tune::packets, INT_MIN, INT_MAX, "packets=0|1|2: never / always / by the probe (default)"},
    {"corun", &Tune::corun, INT_MIN, INT_MAX, "corun=0|1|2: never (the packet kernel in front of k_trace on the group's stream) / by the probe / always"},
    {"cmin", &Tune::cmin, INT_MIN, INT_MAX, "beside k_trace when a probed camera ray enters at least N child boxes"},
    {"cblocks", &Tune::cblocks, INT_MIN, INT_MAX, "fix k_trace's workgroups per CU in such a step (0: 3 or 4 by the step's mix)"},
    {"plog", &Tune::plog, INT_MIN, INT_MAX, "(measurement only): the selector's probe walks packets of 2^N passes x 64 >> N pixels instead of the shape in use"},
    {"pswz", &Tune::pswz, INT_MIN, INT_MAX, "pswz=0|1: k_raygen_packets deals whole 32x32 tiles to the XCDs (workgroup index -> XCD is round robin) instead of consecutive 16-pixel patches: a tile's part of the tree goes through ONE L2 (+0.3-0.7 % on c3 / c2 / c5, profiles/r5ak_packet_xcd.txt)"},
    {"pstep", &Tune::pstep, INT_MIN, INT_MAX, "pstep=0|1: the per-ray step of rounds 4-5 / the interval step where F allows it (default)"},
    {"pstepf", &Tune::pstepf, INT_MIN, INT_MAX, "the interval step while F < N / 100 (0: whatever F is); no report yet: the interval step"},
    {"pprobe", &Tune::pprobe, INT_MIN, INT_MAX, "pprobe=1 (measurement only): the probe's four totals come from a walk with the interval step, so packet_union is what that step enters; decisions are meant to be taken at 0"},
    {"punion", &Tune::punion, INT_MIN, INT_MAX, "packets while U < N / 100 (measured break-even ~2.3: terrain at 1.97 +7..11 %, c5 at 2.07 +3..4 %)"},
    {"fprim", &Tune::fprim, 1, INT_MAX, "chunk size of the work fetch inside the camera rays' part of the index space"},
    {"fgate", &Tune::fgate, INT_MIN, INT_MAX, "... how many such chunks per resident wave that part must hold for it to be used"},
    {"heads", &Tune::heads, 0, 6, "k_trace's work cursors: 2^N ranges of the index space, each with a cursor of its own"},
    {"slow", &Tune::slow, INT_MIN, INT_MAX, "complete what is pending once a pass request has waited N ms (0: never, for tests of the lag itself)"},
    {"ovf", &Tune::ovf, INT_MIN, INT_MAX, "ovf=1|2|3: TEST ONLY - halve one bound so that a queue overflows (1: camera rays, 2: a stage's closest-hit bound, 3: occlusion rays)"},
};
static const size_t kTuneKnobCount = sizeof(kTuneKnobs) / sizeof(kTuneKnobs[0]);

// The tree builder's knobs added after the table above was pinned (tests/host/tune_parse_cpu.cpp holds its 30 rows, their order and
// defaults): same row type, same parser, same rules; a key is looked up in kTuneKnobs first, then here.
static const TuneKnob kTuneBuildKnobs[] = {
    {"sahsub", &Tune::sahsub, 0, 64, "sahsub=0|T: the radix tree's bottom subtrees of at most T triangles are rebuilt by full-sweep SAH (hr_build.hip: k_sah_subtrees; 0: off, one wave holds 64)"},
};
static const size_t kTuneBuildKnobCount = sizeof(kTuneBuildKnobs) / sizeof(kTuneBuildKnobs[0]);

// Items are key=integer (optional sign, decimal digits, nothing after); empty items and an empty string are fine.  An unknown key, a missing
// '=', a value that is no integer or lies outside its row's range is an error: false, with `err` naming the item, and `out` is not to be used.
static bool parseTune(const char *text, Tune &out, std::string &err)
{
    bool seen[kTuneKnobCount + kTuneBuildKnobCount] = {};
    for (const char *p = text; *p;) {
        const std::string item(p, strcspn(p, ","));
        p += item.size() + (p[item.size()] == ',' ? 1 : 0);
        if (item.empty()) continue;
        const size_t eq = item.find('=');
        if (eq == std::string::npos) return err = "'" + item + "' is not key=value", false;
        size_t k = 0;
        auto rowOf = [](size_t i) -> const TuneKnob & { return i < kTuneKnobCount ? kTuneKnobs[i] : kTuneBuildKnobs[i - kTuneKnobCount]; };
        while (k < kTuneKnobCount + kTuneBuildKnobCount && item.compare(0, eq, rowOf(k).key) != 0) ++k;
        if (k == kTuneKnobCount + kTuneBuildKnobCount) return err = "unknown key in '" + item + "'", false;
        const char *v = item.c_str() + eq + 1, *digits = v + (*v == '+' || *v == '-' ? 1 : 0);
        if (!*digits || strspn(digits, "0123456789") != strlen(digits)) return err = "the value in '" + item + "' is not an integer", false;
        errno = 0;
        const long value = strtol(v, nullptr, 10);
        const TuneKnob &row = rowOf(k);
        if (errno == ERANGE || value < row.lo || value > row.hi)
            return err = "the value in '" + item + "' is outside " + std::to_string(row.lo) + ".." + std::to_string(row.hi), false;
        // A repeated key keeps its FIRST value and is no error, as with the strstr parser before this one: bench.py appends
        // ",batch=1" to whatever HR_TUNE its caller set, so a string that names batch twice has to parse.
        if (seen[k]) continue;
        seen[k] = true;
        out.*row.member = (int)value;
        if (row.member == &Tune::blocks) out.blocksSet = true;
    }
    return true;
}
