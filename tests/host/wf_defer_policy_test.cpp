// wf_defer_policy_test.cpp -- the mode of a pipe's shade launches (wf_launch_mode, crt_wf_policy.h; driver invariant I11,
// DESIGN.md 5.10) over hand-built sequences, on the CPU: which launch may leave deferred NEE entries, and that the
// launch behind such a one sweeps the whole pool whatever the tail decision says.  Built and run by
// tests/test_defer_nee_policy_cpu.py; calls no HIP function.
#include <cstdio>

#include "crt_device.h"
#include "crt_wf_policy.h"

using namespace crt;

static int g_failed = 0, g_checked = 0;
#define CHECK(cond)                                                                    \
    do {                                                                               \
        g_checked++;                                                                   \
        if (!(cond)) { g_failed++; std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static bool is(const WfLaunchMode &m, uint32_t tail_bound, uint32_t rearm, uint32_t defer)
{
    return m.tail_bound == tail_bound && m.rearm == rearm && m.defer == defer;
}

// While the host sees work every launch is a pool sweep that re-arms and defers; the option off never defers.
static void test_work_left()
{
    WfPipeView pp;
    for (int k = 0; k < 3; k++) CHECK(is(wf_launch_mode(pp, true, true), 0, 1, 1));
    CHECK(pp.last_defer);
    WfPipeView off;
    for (int k = 0; k < 3; k++) CHECK(is(wf_launch_mode(off, true, false), 0, 1, 0));
    CHECK(!off.last_defer);
}

// The queues run dry and the tail walk is chosen while the last launch deferred: one sweep that neither re-arms nor
// defers, then tail mode -- and tail mode at once where the last launch did not defer.
static void test_run_end()
{
    WfPipeView pp;
    CHECK(is(wf_launch_mode(pp, true, true), 0, 1, 1));
    pp.tail_bound = 128;                                         // (wf_tail_walk, after a status that saw no work left)
    CHECK(is(wf_launch_mode(pp, false, true), 0, 0, 0));         // the sweep: the entries of the launch before are consumed
    CHECK(!pp.last_defer);
    CHECK(is(wf_launch_mode(pp, false, true), 128, 0, 0));
    CHECK(is(wf_launch_mode(pp, false, true), 128, 0, 0));

    WfPipeView dry;                                              // no work left, no tail decision yet: pool mode, kWfDying route
    CHECK(is(wf_launch_mode(dry, true, true), 0, 1, 1));
    CHECK(is(wf_launch_mode(dry, false, true), 0, 0, 0));
    dry.tail_bound = 64;
    CHECK(is(wf_launch_mode(dry, false, true), 64, 0, 0));       // the launch before did not defer: nothing to wait for

    WfPipeView off;
    CHECK(is(wf_launch_mode(off, true, false), 0, 1, 0));
    off.tail_bound = 128;
    CHECK(is(wf_launch_mode(off, false, false), 128, 0, 0));     // option off: the launches of before the option
}

// A tail decision never re-arms, even if the host's view of the queues turns (a new batch resets tail_bound first); the
// sweep it is owed does not defer either, so the rule cannot hold a pipe in pool mode for more than one launch.
static void test_tail_never_rearms()
{
    WfPipeView pp;
    CHECK(is(wf_launch_mode(pp, true, true), 0, 1, 1));
    pp.tail_bound = 256;
    CHECK(is(wf_launch_mode(pp, true, true), 0, 0, 0));
    CHECK(is(wf_launch_mode(pp, true, true), 256, 0, 0));
    pp.tail_bound = 0;                                           // (wf_trace_batch: the next batch's work is there)
    CHECK(is(wf_launch_mode(pp, true, true), 0, 1, 1));
}

int main()
{
    test_work_left();
    test_run_end();
    test_tail_never_rearms();
    std::printf("%d checked, %d failed\n", g_checked, g_failed);
    return g_failed ? 1 : 0;
}
