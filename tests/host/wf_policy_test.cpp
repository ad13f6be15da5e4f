// wf_policy_test.cpp -- the wavefront driver's decisions (crt_wf_policy.h) on hand-built states, on the CPU: two pipes and
// at most three open batches, the smallest set-up in which each rule can go wrong.  Every expected value was worked out
// by hand from the rules as they stood in the driver before they moved into the header.  Built and run by
// tests/test_wf_policy_cpu.py; calls no HIP function.
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

// Two pipes, the batches with ids 0 .. n-1 open since iteration 0, every queue holding work, nothing known yet.
static WfView view(int n_open)
{
    WfView v;
    v.live = true; v.K = 2; v.ring = 4; v.P = 1u << 21; v.Pp = 1u << 20; v.trace_blocks = 256u * 13u;
    for (int i = 0; i < n_open; i++) {
        WfBatch b;
        b.id = (uint32_t)i; b.n = 1; b.last_sample = (uint32_t)i + 1u;
        v.open.push_back(b);
        v.queue_left[i] = true; v.seg_total[i] = 1000000;
    }
    v.work_left = n_open > 0;
    for (int p = 0; p < 2; p++) v.pipes[p].it = v.pipes[p].it_first = v.pipes[p].it_confirmed = v.pipes[p].it_done = 128;
    v.rate_its = 256;
    return v;
}

// The next status record of pipe p (it_end = it_confirmed + 1), every queue still holding work.
static WfStatus status(const WfView &v, int p)
{
    WfStatus st{};
    st.it_end = v.pipes[p].it_confirmed + 1u;
    for (uint32_t b = 0; b < kWfRing; b++) st.left[b] = 1;
    return st;
}

static void test_pool_sizing()
{
    WfOptions o;                                                 // defaults: wf_ring 32, wf_pool_spp 8, wf_pipes 2
    o.tw = 8; o.th = 8;
    WfConfig g = wf_config(o, 1);
    CHECK(g.tiles_x == 1 && g.tiles_y == 1 && g.npix == 64);
    CHECK(g.npix_padded == 64 && g.work_total == 64);
    CHECK(g.K == 1 && g.Pp == 2048 && g.P == 2048);             // capped by 31 x 64 = 1 984, rounded up to a multiple of 256
    CHECK(g.list_cap == 320 && g.work_per_shard == 64 && g.list_per_pipe == 163840);

    o.tw = 1920; o.th = 1080;
    g = wf_config(o, 64);
    CHECK(g.tiles_x == 240 && g.tiles_y == 135 && g.npix == 2073600);
    CHECK(g.npix_padded == 2073600 && g.work_total == 132710400ull);
    CHECK(g.K == 2 && g.Pp == 12582912 && g.P == 25165824);     // capped at 3 * 2^23
    CHECK(g.list_cap == 196864 && g.work_per_shard == 2073600 && g.list_per_pipe == 100794368);

    // one pipe below 2^19 slots, two from there on (a whole number of 16 384-slot strips per pipe)
    o.wf_pool = (1u << 19) - 1u;
    g = wf_config(o, 1);
    CHECK(g.K == 1 && g.Pp == 31u * 16384u && g.P == 31u * 16384u);
    o.wf_pool = 1u << 19;
    g = wf_config(o, 1);
    CHECK(g.K == 2 && g.Pp == 262144 && g.P == 524288);
    o.wf_pipes = 1;
    CHECK(wf_config(o, 1).K == 1 && wf_config(o, 1).Pp == 524288);
    o.wf_pipes = 9;                                              // (at most kWfMaxPipes)
    CHECK(wf_config(o, 1).K == 4);

    // traversal waves per CU: 13 for the ray-ring kernel on the quantised 4-wide tree, else 16; an option overrides both
    WfOptions w;
    CHECK(wf_waves(w) == 16);
    w.quant4_tree = true;
    CHECK(wf_waves(w) == 13);
    w.wf_trace_form = 1;
    CHECK(wf_waves(w) == 16);
    w.wf_waves_per_cu = 7;
    CHECK(wf_waves(w) == 7);
    CHECK(wf_trace_blocks(w, 256) == 1792);
    // k_wf_gen: the option's waves per shard, at most one per 64 list entries, at least one
    CHECK(wf_gen_blocks(w, 196864) == 128 && wf_gen_blocks(w, 320) == 5 && wf_gen_blocks(w, 63) == 1);
}

static void test_batches_and_ring()
{
    WfOptions o;
    o.tw = 1920; o.th = 1080;
    CHECK(wf_batch_cap(o) == 180);                               // 6e9 / (2 073 600 * 16) = 180.8
    CHECK(wf_cohort_size(o, 180) == 16);                         // 2^21 / 2 073 600 = 1: the option as it is
    o.spp_per_launch = 8;
    CHECK(wf_batch_cap(o) == 8 && wf_cohort_size(o, 8) == 8);
    o.spp_per_launch = 0; o.th = 135;                            // the 1/8 share: 2^21 / 259 200 = 8 times as many samples
    CHECK(wf_batch_cap(o) == 256 && wf_cohort_size(o, 256) == 128);
    o.wf_cohort = 1;
    CHECK(wf_cohort_size(o, 256) == 1);
    o.tw = 0;                                                    // (an empty tile counts as one pixel)
    CHECK(wf_batch_cap(o) == 256);

    // ring: the option within 2 .. kWfRing; beyond 4, as many 16-byte staging buffers as fit 32 GB
    WfOptions r;
    CHECK(wf_ring_size(r, 2073600) == 32);
    CHECK(wf_ring_size(r, 132710400) == 15);                     // 15 * 2.123 GB = 31.85 GB, 16 of them 33.97 GB
    CHECK(wf_ring_size(r, (size_t)1 << 40) == 4);
    r.wf_ring = 1;
    CHECK(wf_ring_size(r, 64) == 2);
    r.wf_ring = 100;
    CHECK(wf_ring_size(r, 64) == 32);

    // a live pool is kept unless the batch wants one more than twice as large or small, a larger staging buffer, a
    // ring past the budget, or another kind of work
    WfView v = view(1);
    v.P = 1000000; v.ring = 16;
    CHECK(!wf_must_restart(v, 2000000, 100, 100, false));
    CHECK(wf_must_restart(v, 2000001, 100, 100, false));
    CHECK(!wf_must_restart(v, 500000, 100, 100, false));
    CHECK(wf_must_restart(v, 499999, 100, 100, false));
    CHECK(wf_must_restart(v, 1000000, 101, 100, false));
    CHECK(wf_must_restart(v, 1000000, 100, 100, true));
    CHECK(wf_must_restart(v, 1000000, 132710400, 132710400, false));
    v.ring = 15;
    CHECK(!wf_must_restart(v, 1000000, 132710400, 132710400, false));
}

static void test_status_fold()
{
    // I4: a record from before a batch began (it_end <= from_it) changes nothing about that batch
    WfView v = view(2);
    v.open[1].from_it[0] = v.open[1].from_it[1] = 129;
    WfStatus st = status(v, 0);                                  // it_end 129
    st.left[0] = 0; st.left[1] = 0; st.alive[0] = 7; st.alive[1] = 9; st.consumed[0] = 100; st.consumed[1] = 500;
    st.rays = 77; st.bound = 5;
    wf_fold_status(v, 0, st, true);
    CHECK(v.pipes[0].it_confirmed == 129);
    CHECK(v.pipes[0].dry[0] && !v.queue_left[0] && v.pipes[0].alive_valid[0] && v.pipes[0].alive[0] == 7 && v.consumed[0] == 100);
    CHECK(!v.pipes[0].dry[1] && v.queue_left[1] && !v.pipes[0].alive_valid[1] && v.pipes[0].alive[1] == 0 && v.consumed[1] == 0);
    CHECK(v.consumed_total == 100 && v.work_left);
    CHECK(v.pipes[0].rays == 77 && v.pipes[0].bound == 5);
    CHECK(!v.pipes[0].any);                                      // not newer than the newest batch's from_it
    CHECK(!v.pipes[1].dry[0] && !v.pipes[1].alive_valid[0]);    // (the other pipe's own view is its own)

    // dry never turns back, a smaller `consumed` is ignored, alive follows only a record that counted
    st = status(v, 0);                                           // it_end 130: newer than batch 1's from_it
    st.left[0] = 1; st.alive[0] = 3; st.consumed[0] = 50; st.consumed[1] = 20;
    wf_fold_status(v, 0, st, false);
    CHECK(v.pipes[0].dry[0] && !v.queue_left[0]);
    CHECK(v.consumed[0] == 100 && v.consumed[1] == 20 && v.consumed_total == 120);
    CHECK(v.pipes[0].alive[0] == 7 && !v.pipes[0].alive_valid[1]);
    CHECK(v.pipes[0].any && !v.pipes[1].any);

    // per_it: half the old estimate, half the work per iteration since the last sample -- only while work is left
    // and only when iterations advanced
    v = view(1);
    v.per_it = 1000.0;
    st = status(v, 0);
    st.consumed[0] = 300;
    wf_fold_status(v, 0, st, false);
    CHECK(v.per_it == 650.0 && v.rate_its == 257 && v.rate_consumed == 300);
    st = status(v, 1);
    st.consumed[0] = 300;                                        // nothing consumed meanwhile: the estimate stays, the sample point moves
    wf_fold_status(v, 1, st, false);
    CHECK(v.per_it == 650.0 && v.rate_its == 258 && v.rate_consumed == 300);
    st = status(v, 0);
    st.consumed[0] = 900; st.left[0] = 0;                        // the queue ran dry: no sample
    wf_fold_status(v, 0, st, false);
    CHECK(!v.work_left && v.per_it == 650.0 && v.rate_its == 259 && v.rate_consumed == 900);
    v = view(1);
    v.per_it = 1000.0; v.rate_its = 1000;                        // (iterations did not advance past the sample point)
    st = status(v, 0);
    st.consumed[0] = 300;
    wf_fold_status(v, 0, st, false);
    CHECK(v.per_it == 1000.0 && v.rate_its == 1000 && v.rate_consumed == 0);
}

// Three open batches; both pipes have seen the queues of the two oldest dry and counted `a0`, `a1` paths of each.
static WfView evict_view(uint32_t a0, uint32_t a1)
{
    WfView v = view(3);
    for (int p = 0; p < 2; p++)
        for (int b = 0; b < 3; b++) { v.pipes[p].dry[b] = true; v.pipes[p].alive_valid[b] = true; }
    for (int b = 0; b < 3; b++) { v.pipes[0].alive[b] = a0; v.pipes[1].alive[b] = a1; }
    return v;
}

static void test_eviction()
{
    WfOptions o;                                                 // wf_finish_at 32 768
    WfView v = evict_view(10, 30);
    wf_decide_evictions(v, o);
    CHECK(v.open[0].evicting && v.open[1].evicting && !v.open[2].evicting);       // the newest is never evicted
    CHECK(v.open[0].need_mask == 3 && v.open[0].evict_bound == 30 && v.open[0].launched_mask == 0);
    CHECK(v.pipes[0].evict_next == 3 && v.pipes[1].evict_next == 3);              // batch ids 0 and 1

    // not while one pipe that is not done lacks alive_valid or dry -- and order is kept: nothing behind it either
    v = evict_view(10, 30);
    v.pipes[1].dry[0] = false;
    wf_decide_evictions(v, o);
    CHECK(!v.open[0].evicting && !v.open[1].evicting && v.pipes[0].evict_next == 0 && v.pipes[1].evict_next == 0);
    v = evict_view(10, 30);
    v.pipes[0].alive_valid[0] = false;
    wf_decide_evictions(v, o);
    CHECK(!v.open[0].evicting && !v.open[1].evicting);
    v.open[0].evicting = true;                                   // (one already on its way does not hold the next up)
    wf_decide_evictions(v, o);
    CHECK(v.open[1].evicting && v.pipes[0].evict_next == 2 && v.pipes[1].evict_next == 2);

    // a done pipe is skipped: nothing is asked of it, nothing is evicted from it
    v = evict_view(10, 30);
    v.pipes[1].done = true; v.pipes[1].dry[0] = false; v.pipes[1].alive_valid[0] = false;
    wf_decide_evictions(v, o);
    CHECK(v.open[0].evicting && v.open[0].need_mask == 1 && v.open[0].evict_bound == 10);
    CHECK(v.pipes[0].evict_next == 3 && v.pipes[1].evict_next == 0);

    // need_mask holds only pipes with alive > 0; none alive at all: an eviction with mask 0
    v = evict_view(0, 30);
    wf_decide_evictions(v, o);
    CHECK(v.open[0].evicting && v.open[0].need_mask == 2 && v.open[0].evict_bound == 30 && v.pipes[0].evict_next == 0);
    v = evict_view(0, 0);
    o.wf_finish_at = 0;                                          // (0 = never move paths -- but there are none)
    wf_decide_evictions(v, o);
    CHECK(v.open[0].evicting && v.open[0].need_mask == 0 && v.open[0].evict_bound == 0 && v.open[1].evicting);
    v = evict_view(1, 0);
    wf_decide_evictions(v, o);
    CHECK(!v.open[0].evicting);

    // too many paths: more than a side pool holds in one pipe, or more than min(wf_finish_at, kWfSideCap) * K in all
    o.wf_finish_at = 1u << 30;
    v = evict_view(kWfSideCap + 1u, 0);
    wf_decide_evictions(v, o);
    CHECK(!v.open[0].evicting && !v.open[1].evicting);
    v = evict_view(kWfSideCap, kWfSideCap);
    wf_decide_evictions(v, o);
    CHECK(v.open[0].evicting && v.open[0].evict_bound == kWfSideCap);
    o.wf_finish_at = 100;
    v = evict_view(150, 51);
    wf_decide_evictions(v, o);
    CHECK(!v.open[0].evicting);
    v = evict_view(150, 50);
    v.pipes[0].alive[1] = 151;                                   // batch 0 fits (200), batch 1 does not (201)
    wf_decide_evictions(v, o);
    CHECK(v.open[0].evicting && !v.open[1].evicting && v.pipes[0].evict_next == 1 && v.pipes[1].evict_next == 1);

    // all_evicting: the flush has sent everything to the side pools already
    v = evict_view(10, 30);
    v.all_evicting = true;
    wf_decide_evictions(v, o);
    CHECK(!v.open[0].evicting && v.pipes[0].evict_next == 0);
}

static void test_flush_decisions()
{
    WfOptions o;                                                 // wf_flush_at 4 096, wf_tail_walk 1
    // drained (I10): no work left, a status since the newest batch began, no rays -- and the pipe's OWN word that
    // every open batch's queue is dry
    WfView v = view(2);
    v.work_left = false; v.queue_left[0] = v.queue_left[1] = false;
    v.pipes[0].any = true; v.pipes[0].rays = 0; v.pipes[0].dry[0] = true; v.pipes[0].dry[1] = false;
    v.pipes[1].dry[0] = v.pipes[1].dry[1] = true;                // (the other pipe's records do not count)
    CHECK(!wf_pipe_drained(v, 0));
    v.pipes[0].dry[1] = true;
    CHECK(wf_pipe_drained(v, 0));
    v.pipes[0].rays = 1;
    CHECK(!wf_pipe_drained(v, 0));
    v.pipes[0].rays = 0; v.pipes[0].any = false;
    CHECK(!wf_pipe_drained(v, 0));
    v.pipes[0].any = true; v.work_left = true;
    CHECK(!wf_pipe_drained(v, 0));

    // tail walk: rays < min(Pp / 4, 65 536); tail_bound = max(64, bound rounded up to 64); blocks_now = rays / 32 + 64
    // within [64, trace_blocks]
    v = view(1);
    v.work_left = false; v.pipes[0].any = true; v.pipes[0].rays = 65535; v.pipes[0].bound = 1030;
    CHECK(wf_tail_walk(v, o, 0));
    CHECK(v.pipes[0].tail_bound == 1088 && v.pipes[0].blocks_now == 65535 / 32 + 64);
    v.pipes[0].rays = 65536; v.pipes[0].tail_bound = 0;
    CHECK(!wf_tail_walk(v, o, 0) && v.pipes[0].tail_bound == 0);
    v.Pp = 4096; v.pipes[0].rays = 1024;                         // Pp / 4
    CHECK(!wf_tail_walk(v, o, 0));
    v.pipes[0].rays = 1023; v.pipes[0].bound = 0;
    CHECK(wf_tail_walk(v, o, 0) && v.pipes[0].tail_bound == 64 && v.pipes[0].blocks_now == 64 + 31);
    v.pipes[0].bound = 64; v.trace_blocks = 80;
    CHECK(wf_tail_walk(v, o, 0) && v.pipes[0].tail_bound == 64 && v.pipes[0].blocks_now == 80);
    v.pipes[0].any = false; v.pipes[0].tail_bound = 0;
    CHECK(!wf_tail_walk(v, o, 0));
    v.pipes[0].any = true; v.work_left = true;
    CHECK(!wf_tail_walk(v, o, 0));
    v.work_left = false; o.wf_tail_walk = 0;
    CHECK(!wf_tail_walk(v, o, 0) && v.pipes[0].tail_bound == 0);
    o.wf_tail_walk = 1;

    // flush-all: every pipe that is not done has a status and lists at most min(wf_flush_at, kWfSideCap) rays
    v = view(3);
    v.work_left = false;
    v.pipes[0].any = v.pipes[1].any = true; v.pipes[0].rays = 4096; v.pipes[1].rays = 4097;
    CHECK(!wf_flush_all_ready(v, o));
    v.pipes[1].rays = 4096;
    CHECK(wf_flush_all_ready(v, o));
    v.pipes[1].any = false;
    CHECK(!wf_flush_all_ready(v, o));
    v.pipes[1].done = true; v.pipes[1].rays = 1u << 20;          // (a done pipe is not asked)
    CHECK(wf_flush_all_ready(v, o));
    v.work_left = true;
    CHECK(!wf_flush_all_ready(v, o));
    v.work_left = false; o.wf_flush_at = 0;                      // 0 = never
    CHECK(!wf_flush_all_ready(v, o));
    o.wf_flush_at = 1u << 30; v.pipes[0].rays = kWfSideCap + 1u; // (never more than a side pool holds)
    CHECK(wf_flush_at(o) == kWfSideCap && !wf_flush_all_ready(v, o));
    v.pipes[0].rays = kWfSideCap;
    CHECK(wf_flush_all_ready(v, o));
    CHECK(wf_open_mask(v) == 7);                                 // the mask names every open batch
    v.open.erase(v.open.begin());
    CHECK(wf_open_mask(v) == 6);
}

static void test_feed()
{
    WfOptions o;                                                 // wf_feed 1, wf_chunk 1
    WfView v = view(3);
    v.consumed[0] = 400000; v.consumed[1] = 1000000; v.queue_left[2] = false;    // 600 000 + nothing + a dry queue
    v.per_it = 50000.0;
    WfFeed f = wf_feed(v, o, 4);
    CHECK(f.backlog == 600000 && f.per_it == 50000.0 && f.need == 400000.0);
    CHECK(wf_feed_iters(v, o, f) == 1);                          // ceil(400 000 / 50 000 / 2) = 4, clamped to wf_chunk
    o.wf_chunk = 16;
    CHECK(wf_feed_iters(v, o, f) == 4);
    o.wf_chunk = 3;
    CHECK(wf_feed_iters(v, o, f) == 3);
    o.wf_feed = 2.5;
    f = wf_feed(v, o, 4);
    CHECK(f.need == 100000.0 && wf_feed_iters(v, o, f) == 1);
    f = wf_feed(v, o, 5);
    CHECK(f.need == -25000.0);                                   // (the driver enqueues nothing unless need > 0)
    v.per_it = 10.0; o.wf_feed = 1.0;                            // the estimate counts as 1 024 at least
    f = wf_feed(v, o, 100);
    CHECK(f.per_it == 1024.0 && f.need == 600000.0 - 102400.0);
    v.consumed[0] = 999999; v.K = 2;
    f = wf_feed(v, o, 0);
    CHECK(f.backlog == 1 && f.need == 1.0 && wf_feed_iters(v, o, f) == 1);       // at least one iteration
}

int main()
{
    test_pool_sizing();
    test_batches_and_ring();
    test_status_fold();
    test_eviction();
    test_flush_decisions();
    test_feed();
    std::printf("%d checks, %d failed\n", g_checked, g_failed);
    return g_failed ? 1 : 0;
}
