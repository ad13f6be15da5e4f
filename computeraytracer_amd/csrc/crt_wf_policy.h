// crt_wf_policy.h -- what the wavefront driver KNOWS, apart from what it does: the host's view of the pool (pipes, open
// batches, queues) and every decision taken from it, as plain functions over plain structs.  No function here calls
// the HIP runtime, so the rules can be exercised on the CPU (tests/host/wf_policy_test.cpp); the driver
// (crt_wf_driver.cpp) keeps every stream, event, launch, wait, watchdog and error path and calls these at the points
// where the decisions fall.  Everything that sizes a launch (the pool, the lists, the traversal waves, the ring)
// lives here too.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

#include "crt_device.h"

namespace crt {

constexpr int kWfMaxPipes = 4;      // up to this many half-pools, each its own shade->trace chain on its own stream
constexpr int kStatusRing = 64;     // status records per pipe (one per iteration in flight)

// The options and the state of the context that the decisions read (wf_options fills it from crt_ctx).
struct WfOptions {
    uint32_t tw = 0, th = 0;        // the tile
    uint32_t wf_pool = 0, wf_waves_per_cu = 0, spp_per_launch = 0;   // 0 = auto
    int wf_pool_spp = 8, wf_ring = 32, wf_pipes = 2, wf_trace_form = 2, wf_cohort = 16, wf_chunk = 1, wf_tail_walk = 1, wf_gen_blocks = 128;
    int wf_affinity = 0;            // region-major work shards (crt_work_map.h)
    uint32_t wf_finish_at = 32768, wf_flush_at = 4096;
    double wf_feed = 1.0;
    bool quant4_tree = false;       // the walked tree is the quantised 4-wide one (bvh4q.ok && !bvh8q.ok)
};

// ---------------------------------------------------------------- the view
// One shade->trace chain over its share of the pool, as the host sees it.
struct WfPipeView {
    uint32_t it = 0;                // the next iteration to enqueue (numbers are never reused: a run starts where the last one
    uint32_t it_first = 0;          // ended, so a late status write of the last run cannot be taken for one of this run)
    uint32_t it_confirmed = 0;      // iterations < it_confirmed are known to have completed (a status of them was read)
    uint32_t it_done = 0;           // iterations < it_done are known to have completed (their traversal launch's event has)
    uint32_t chunk = 2, tail_bound = 0, blocks_now = 0;
    // Status records: iteration i's is written by the shade launch of iteration i + 1 into slot i % kStatusRing and
    // is pending while it_confirmed <= i < it.
    bool st_counted[kStatusRing] = {};      // that iteration's shade launch counted the alive paths per batch
    bool done = false;              // flush: nothing more is enqueued for this pipe (drained or emptied by eviction)
    bool any = false;               // a status has been read since the newest batch began
    unsigned long long rays = 0;    // from the last status: rays listed by its last iteration
    uint32_t bound = 0;             // ... and the most rays one shard listed
    uint32_t alive[kWfRing] = {};   // per batch id, from this pipe's last status that counted: paths alive in its pool
    bool alive_valid[kWfRing] = {};
    bool dry[kWfRing] = {};         // a status of this pipe saw that batch's queue empty (its OWN view: its count of
                                    // alive paths only bounds the future once no more such paths can start here)
    uint32_t evict_next = 0;        // evict_mask for the next shade launch
    bool last_defer = false;        // the last shade launch enqueued for this pipe could leave deferred NEE entries (WfParams::defer)
};

// A batch of samples whose paths are (or may still be) in flight.
struct WfBatch {
    uint32_t n = 0, last_sample = 0, id = 0;
    uint32_t from_it[kWfMaxPipes] = {};   // per pipe: chunks enqueued from this iteration on know the batch
    bool ready = true;              // its queue has been reset on the device (ev_pub[id] seen complete): launches may list it
    uint32_t evict_bound = 0;       // the most paths one pipe held when the eviction was decided (sizes the finish launch)
    bool evicting = false;          // its last paths are being moved to the side pools (or none are left)
    uint32_t need_mask = 0;         // pipes whose next shade launch evicts ...
    uint32_t launched_mask = 0;     // ... and those that have enqueued it (ev_evict[p][id] recorded)
    uint32_t as_commit = 0;         // adaptive: the last batch of its crt_trace_adaptive call adds this many samples to the
                                    // active tiles' counts after its resolve (last_sample is then the call's samples so far)
};

struct WfView {
    bool live = false;              // the pipes are forked and hold (or may hold) paths
    int K = 0;
    uint32_t P = 0, Pp = 0, list_cap = 0, trace_blocks = 0, ring = 4;
    uint32_t seg_wps[kWfRing] = {};             // per batch id: work items per shard / in total
    unsigned long long seg_total[kWfRing] = {};
    WfPipeView pipes[kWfMaxPipes];
    std::vector<WfBatch> open;                  // unresolved batches, oldest first; back() = the newest
    bool queue_left[kWfRing] = {};              // that batch's queue still holds work (latest knowledge of any pipe)
    unsigned long long consumed[kWfRing] = {};  // work items taken from it (latest knowledge)
    unsigned long long consumed_total = 0;      // ... summed over all batches since the pool started
    bool work_left = false;                     // any open batch's queue holds work
    double per_it = 0.0;                        // work items one iteration of one pipe consumes while work is there (estimate)
    unsigned long long rate_consumed = 0;       // sample point of that estimate
    unsigned long long rate_its = 0;
    uint32_t listed_until[kWfRing][kWfMaxPipes] = {};   // per id and pipe: launches of iterations < this may look at that queue
    bool resolved_recorded[kWfRing] = {};       // ev_resolved[id] has been recorded since the pool started
    bool all_evicting = false;                  // flush: everything alive was sent to the side pools
    int poll_next = 0;                          // round robin over the pipes for blocking waits
};

// ---------------------------------------------------------------- sizes
// persistent traversal waves per CU and pipe: 13 for k_wf_trace2, 16 for k_wf_trace (profiles/r03_ab_waves.txt)
inline uint32_t wf_waves(const WfOptions &o) { return o.wf_waves_per_cu ? o.wf_waves_per_cu : (o.wf_trace_form == 2 && o.quant4_tree) ? 13u : 16u; }

// k_wf_trace's grid per pipe; k_wf_gen's waves per shard (each takes every gen_blocks-th chunk of 64 dead slots of its shard's list)
inline uint32_t wf_trace_blocks(const WfOptions &o, int num_cu) { return (uint32_t)num_cu * wf_waves(o); }
inline uint32_t wf_gen_blocks(const WfOptions &o, uint32_t list_cap) { return std::max(1u, std::min((uint32_t)o.wf_gen_blocks, list_cap / 64u)); }

struct WfConfig {
    uint32_t tiles_x, tiles_y, npix_padded, P, Pp, list_cap, work_per_shard;
    uint32_t map_samples;           // WfSeg::map_samples: n under "wf_affinity" (the shards' sizes are then wm_shard_size's), else 0
    int K;
    unsigned long long work_total;
    size_t npix, list_per_pipe;
};

inline WfConfig wf_config(const WfOptions &o, uint32_t n)
{
    WfConfig g{};
    g.tiles_x = (o.tw + 7) / 8; g.tiles_y = (o.th + 7) / 8;
    g.npix_padded = g.tiles_x * g.tiles_y * 64u;
    g.npix = (size_t)o.tw * o.th;
    g.work_total = (unsigned long long)n * g.npix_padded;
    // pool: between 1 M and 24 M slots, about a quarter of a LARGE batch's paths and at least wf_pool_spp (8) per tile
    // pixel; a stream of small batches shares the pool, so it is sized by the tile, not by one call's samples.  (8 M was
    // the cap while the pool's streams still washed the scene out of the L2 with every launch; with them non-temporal a
    // launch costs what its rays cost plus a fixed ramp-up, tail and gap, and larger launches amortise those:
    // profiles/r02_pool_sweep.txt, r02_pool_bench.txt -- 8 / 16 / 24 M slots: 63.9 / 61.4 / 60.5 ms per 64-spp step,
    // 1.035 / 1.001 / 1.007 ms per 1-spp step.)
    const unsigned long long per_pixel = std::max<unsigned long long>(g.work_total / 4u, (unsigned long long)g.npix_padded * (unsigned long long)o.wf_pool_spp);
    uint32_t P = o.wf_pool ? o.wf_pool : (uint32_t)std::min<unsigned long long>(3u << 23, std::max<unsigned long long>(1u << 20, per_pixel));
    // (a pool may exceed one batch's work: several batches share it, but never more than the ring holds)
    const unsigned long long most = g.work_total * (unsigned long long)std::max(1u, std::min<uint32_t>(o.wf_ring, kWfRing) - 1u);
    if ((unsigned long long)P > most) P = (uint32_t)most;
    // Two (or more) half-pools on separate streams: one half's shade pass (an HBM stream) overlaps
    // the other half's traversal (latency-bound).  Small pools keep one pipe.
    int K = std::max(1, std::min(o.wf_pipes, kWfMaxPipes));
    if (P < (1u << 19)) K = 1;
    // slots per pipe: a whole number of shade blocks for every one of the 64 shards when possible
    // (measured: a 1/8 strip takes 13.0 ms with such a pool and 15.1 ms with one 0.4 % smaller)
    uint32_t Pp = P / (uint32_t)K;
    Pp = Pp >= 16384u ? (Pp / 16384u) * 16384u : ((Pp + 255u) & ~255u);
    g.K = K; g.Pp = Pp; g.P = Pp * (uint32_t)K;
    // list capacity per shard: any shade block size >= 64 maps at most ceil(blocks/shards) blocks to a shard
    g.list_cap = ((Pp / 64u + kWfShards - 1) / kWfShards) * 64u + 256u;
    g.work_per_shard = (uint32_t)((g.work_total + kWfShards - 1) / kWfShards);
    g.work_per_shard = (g.work_per_shard + 63u) & ~63u;
    g.map_samples = o.wf_affinity ? n : 0u;
    g.list_per_pipe = (size_t)8 * g.list_cap * kWfShards;                 // [2 parities][4 classes]
    return g;
}

// Samples per batch at most: the staging buffer stays below ~6 GB and work ids fit 32 bits.
inline uint32_t wf_batch_cap(const WfOptions &o)
{
    const size_t npix = std::max<size_t>((size_t)o.tw * o.th, 1);
    uint32_t cap = (uint32_t)std::max<size_t>(1, std::min<size_t>(256, (size_t)6e9 / (npix * 16)));
    if (o.spp_per_launch) cap = std::min(cap, o.spp_per_launch);
    return cap;
}

// A cohort is wf_cohort samples of a 2-Mpixel frame's worth of paths; a smaller tile (the row-band share of a
// multi-GPU run) takes proportionally more samples, up to 8 times (measured on the 1/8 share of the 1080p frame,
// 64 spp per call: 8.48 ms per call with every call its own batch, 7.94 ms with two calls per batch).
inline uint32_t wf_cohort_size(const WfOptions &o, uint32_t cap)
{
    const size_t npix = std::max<size_t>((size_t)o.tw * o.th, 1);
    const uint32_t scale = (uint32_t)std::min<size_t>(8, std::max<size_t>(1, ((size_t)1 << 21) / npix));
    return o.wf_cohort <= 1 ? 1u : std::min<uint32_t>(cap, (uint32_t)o.wf_cohort * scale);
}

// batches in flight at most: the staging buffers (one per batch id, staging_elems float4 each) stay within ~32 GB
inline bool wf_ring_over_budget(uint32_t ring, size_t staging_elems) { return ring > 4u && (double)ring * (double)staging_elems * 16.0 > 32.0e9; }

inline uint32_t wf_ring_size(const WfOptions &o, size_t staging_elems)
{
    uint32_t ring = std::max(2u, std::min<uint32_t>(o.wf_ring, kWfRing));
    while (wf_ring_over_budget(ring, staging_elems)) ring--;
    return ring;
}

// A live pool is kept as it is unless this batch wants one more than twice as large or small (e.g. 64-spp calls
// after 1-spp calls), or the staging buffers are too small.
// The staging buffers are never reallocated under a live pool (the pipes hold their addresses, batches in flight
// their contents): if ANY buffer of the ring is too small for this batch (staging_min: the smallest of them), or the
// ring would take the buffers past the 32 GB budget at this batch's size, the pool is run to its end first and set up
// afresh.  other_kind: the batch is adaptive and the pool uniform or the reverse, or over another set of tiles (one kind
// of work per pool).
inline bool wf_must_restart(const WfView &v, uint32_t want_P, size_t staging_elems, size_t staging_min, bool other_kind)
{
    const bool regrow = staging_min < staging_elems || wf_ring_over_budget(v.ring, staging_elems) || other_kind;
    return (unsigned long long)want_P > 2ull * v.P || 2ull * want_P < (unsigned long long)v.P || regrow;
}

// ---------------------------------------------------------------- one status record of pipe p, folded into the view
// (the caller has checked it_end == it_confirmed + 1 and `dropped`; counted: that iteration's shade launch counted)
inline void wf_fold_status(WfView &r, int p, const WfStatus &st, bool counted)
{
    WfPipeView &pp = r.pipes[p];
    pp.it_confirmed = st.it_end;
    for (const WfBatch &b : r.open) {
        if (st.it_end <= b.from_it[p]) continue;                 // from before that batch began: knows nothing about it
        const uint32_t id = b.id;
        if (!st.left[id]) { pp.dry[id] = true; r.queue_left[id] = false; }      // (monotone within a batch)
        if (counted) { pp.alive[id] = st.alive[id]; pp.alive_valid[id] = true; }
        if (st.consumed[id] > r.consumed[id]) { r.consumed_total += st.consumed[id] - r.consumed[id]; r.consumed[id] = st.consumed[id]; }
    }
    r.work_left = false;
    for (const WfBatch &b : r.open) r.work_left = r.work_left || r.queue_left[b.id];
    pp.rays = st.rays; pp.bound = st.bound;
    if (!r.open.empty() && st.it_end > r.open.back().from_it[p]) pp.any = true;
    // work one iteration of one pipe consumes: sampled over intervals at whose end work was still there
    unsigned long long its = 0;
    for (int q = 0; q < r.K; q++) its += r.pipes[q].it_confirmed;
    if (its > r.rate_its) {
        if (r.work_left && r.consumed_total > r.rate_consumed) {
            const double sample = (double)(r.consumed_total - r.rate_consumed) / (double)(its - r.rate_its);
            r.per_it = 0.5 * r.per_it + 0.5 * sample;
        }
        r.rate_its = its; r.rate_consumed = r.consumed_total;
    }
}

// ---------------------------------------------------------------- retirement
// Retirement decisions after a status: the oldest batches (never the newest -- flush does that one) whose queue is
// dry for every pipe and of which few paths are left (alive slots only shrink once the queue is dry, so they still
// fit when the launch runs) have them evicted by every pipe's next shade launch; none left: nothing to evict.
inline void wf_decide_evictions(WfView &r, const WfOptions &o)
{
    if (r.all_evicting) return;
    const unsigned long long evict_at = std::min<unsigned long long>(o.wf_finish_at, kWfSideCap);
    for (size_t i = 0; i + 1 < r.open.size(); i++) {
        WfBatch &b = r.open[i];
        if (b.evicting) continue;
        bool ready = true;
        unsigned long long tot = 0, mx = 0;
        uint32_t mask = 0;
        for (int p = 0; p < r.K; p++) {
            const WfPipeView &pp = r.pipes[p];
            if (pp.done) continue;                               // (a drained pipe holds no path at all)
            ready = ready && pp.alive_valid[b.id] && pp.dry[b.id];
            tot += pp.alive[b.id]; mx = std::max<unsigned long long>(mx, pp.alive[b.id]);
            if (pp.alive[b.id]) mask |= 1u << p;
        }
        if (!ready) break;                                       // in order
        if (tot != 0 && !(mx <= kWfSideCap && tot <= evict_at * (unsigned)r.K)) break;
        b.evicting = true; b.need_mask = mask; b.launched_mask = 0; b.evict_bound = (uint32_t)mx;
        for (int p = 0; p < r.K; p++) if ((mask >> p) & 1u) r.pipes[p].evict_next |= 1u << b.id;
    }
}

// ---------------------------------------------------------------- feeding (wf_pump)
// How much published work the iterations in flight will not consume: `inflight` iterations over all pipes.
struct WfFeed {
    unsigned long long backlog;
    double per_it, need;            // need > 0: enqueue more
};

inline WfFeed wf_feed(const WfView &r, const WfOptions &o, unsigned long long inflight)
{
    WfFeed f{};
    for (const WfBatch &b : r.open)
        if (r.queue_left[b.id] && r.seg_total[b.id] > r.consumed[b.id]) f.backlog += r.seg_total[b.id] - r.consumed[b.id];
    f.per_it = std::max(r.per_it, 1024.0);
    f.need = (double)f.backlog - f.per_it * (double)inflight * o.wf_feed;
    return f;
}

// ... and how many iterations the chosen pipe gets for it
inline uint32_t wf_feed_iters(const WfView &r, const WfOptions &o, const WfFeed &f)
{
    const double want = std::ceil(f.need / f.per_it / (double)r.K);
    return (uint32_t)std::min<double>((double)o.wf_chunk, std::max(1.0, want));
}

// ---------------------------------------------------------------- the flush (wf_finish_all), after a status of pipe p
// Every alive slot lists a ray: no rays and no work means this pipe is drained (another pipe's view of the queues can
// lag; a pipe with no rays while work may be left simply keeps going) -- but only on its OWN word that every queue is
// dry (I10): r.work_left may have turned false through another pipe's status, and a gen launch of this pipe behind the
// record just read may have been the one that took, and culled, the last chunks.  wf_decide_evictions asks nothing of a
// drained pipe, so its own record has to say it here.
inline bool wf_pipe_drained(const WfView &r, int p)
{
    const WfPipeView &pp = r.pipes[p];
    bool own_dry = true;
    for (const WfBatch &b : r.open) own_dry = own_dry && pp.dry[b.id];
    return !r.work_left && pp.any && pp.rays == 0 && own_dry;
}

// The tail: no path can start any more, so ray counts only shrink from here.  Shade walks the ray lists instead of
// the whole pool and the grids shrink.  Per-shard bound for later iterations: slots never change shard and none are
// re-armed once the queues are empty, so no list of a shard can ever grow beyond the slots alive in it now.
inline bool wf_tail_walk(WfView &r, const WfOptions &o, int p)
{
    WfPipeView &pp = r.pipes[p];
    if (!(!r.work_left && pp.any && o.wf_tail_walk && pp.rays < std::min<unsigned long long>((unsigned long long)r.Pp / 4u, 65536ull))) return false;
    pp.tail_bound = std::max<uint32_t>(64u, (pp.bound + 63u) & ~63u);
    pp.blocks_now = (uint32_t)std::min<unsigned long long>(r.trace_blocks, std::max<unsigned long long>(64, pp.rays / 32u + 64u));
    return true;
}

// The mode of pipe pp's next shade launch (wf_enqueue asks once per launch).  rearm: dead slots are listed and a k_wf_gen
// launch follows -- in pool mode, while the host sees work in a queue.  defer: the launch may leave deferred NEE entries
// (option "wf_defer_nee"); a slot freed early is worth something only while there is work to put into
// it.  I11 of crt_wf_driver.cpp: the launch behind one that deferred visits EVERY slot of the pool -- tail mode, which
// walks the ray lists, waits one iteration (a sweep that neither re-arms nor defers).
struct WfLaunchMode { uint32_t tail_bound, rearm, defer; };
inline WfLaunchMode wf_launch_mode(WfPipeView &pp, bool work_left, bool defer_nee)
{
    WfLaunchMode m;
    m.tail_bound = pp.last_defer ? 0u : pp.tail_bound;
    m.rearm = (pp.tail_bound == 0u && work_left) ? 1u : 0u;
    m.defer = (m.rearm && defer_nee) ? 1u : 0u;
    pp.last_defer = m.defer != 0u;
    return m;
}

inline unsigned long long wf_flush_at(const WfOptions &o) { return std::min<unsigned long long>(o.wf_flush_at, kWfSideCap); }

// once few paths are left altogether, everything alive goes to the side pools and the pool is done
inline bool wf_flush_all_ready(const WfView &r, const WfOptions &o)
{
    const unsigned long long flush_at = wf_flush_at(o);
    if (!(!r.work_left && flush_at > 0)) return false;
    bool ready = true;
    for (int q = 0; q < r.K; q++) {
        if (r.pipes[q].done) continue;
        ready = ready && r.pipes[q].any && r.pipes[q].rays <= flush_at;
    }
    return ready;
}

// (its eviction mask: every open batch)
inline uint32_t wf_open_mask(const WfView &r)
{
    uint32_t mask = 0;
    for (const WfBatch &b : r.open) mask |= 1u << b.id;
    return mask;
}

}  // namespace crt
