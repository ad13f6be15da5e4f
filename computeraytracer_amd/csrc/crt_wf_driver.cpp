// crt_wf_driver.cpp -- the host side of the wavefront pipeline (crt_wavefront.hip): every stream, event, launch and wait.
// What it decides from the statuses that come back is in crt_wf_policy.h.
#include <chrono>
#include <thread>

#include "crt_ctx.h"

using namespace crt;

namespace crt {

// ---------------------------------------------------------------- wavefront driver
//
// The pool (crt_wavefront.hip) is a steady-state machine: every iteration of a pipe is one shade launch (advance
// every path slot by one bounce, re-arm dead slots from the work queues) and one traversal launch.  The host's
// part is to keep it fed and to retire finished batches:
//
//   publish   a crt_trace call becomes a BATCH: a work queue, a staging buffer and side pools of its own, indexed by
//             the batch id that a path carries in its flags.  Up to `ring` batches are in flight.
//   pump      enqueue as many iterations as the published work needs -- by an estimate of how many work items one
//             iteration consumes, corrected by every status that comes back -- and return.  The call does NOT wait
//             for its work: statuses are polled (hipEventQuery), the only blocking waits are back-pressure (the
//             ring of batches or of status buffers is full).  A loop of 1-spp calls (the reference's frame loop,
//             main.js:597-611) therefore runs the pool exactly like one large batch does.
//   retire    batches resolve in order (the accumulator is summed in sample order).  A batch whose queue is dry
//             for every pipe and of which few paths are left has those EVICTED by the pipes' next shade launch into
//             side pools; k_wf_finish runs them to their end (one launch for all pipes and every batch that is ready)
//             and k_wf_resolve adds the batch to the accumulator -- on the context's stream, under the pool's work.
//   flush     crt_sync and every call that reads or changes state: run everything to its end.
//
//   cohorts   small calls are merged: crt_trace only notes their samples, which become one batch once wf_cohort of
//             them have come together (wf_publish_pending) -- a batch of many samples per pixel keeps the paths in
//             flight inside a band of the image.
//
// What the driver needs to know about an iteration (queue cursors, rays listed, paths alive per batch) is written
// into a pinned host record by the first wave of the NEXT iteration's shade launch (write_status) and polled here.

// What the decisions of crt_wf_policy.h read of the context.
WfOptions wf_options(const crt_ctx *c)
{
    WfOptions o;
    o.tw = c->tw; o.th = c->th;
    o.wf_pool = c->wf_pool; o.wf_waves_per_cu = c->wf_waves_per_cu; o.spp_per_launch = c->spp_per_launch;
    o.wf_pool_spp = c->wf_pool_spp; o.wf_ring = c->wf_ring; o.wf_pipes = c->wf_pipes; o.wf_trace_form = c->wf_trace_form;
    o.wf_cohort = c->wf_cohort; o.wf_chunk = c->wf_chunk; o.wf_tail_walk = c->wf_tail_walk; o.wf_gen_blocks = c->wf_gen_blocks;
    o.wf_affinity = c->wf_affinity;
    o.wf_finish_at = c->wf_finish_at; o.wf_flush_at = c->wf_flush_at; o.wf_feed = c->wf_feed;
    o.quant4_tree = c->bvh4q.ok && !c->bvh8q.ok;
    return o;
}

// The deep-stack overflow area: wf_overflow_levels levels beyond the LDS part for every resident traversal lane of every
// pipe ([pipe][level][lane]; pipe p's part starts at p * lanes per pipe * levels).
int wf_ensure_overflow(crt_ctx *c)
{
    if (c->num_cu == 0) {
        hipDeviceProp_t prop;
        HIPCHK(c, hipGetDeviceProperties(&prop, c->device));
        c->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    const size_t lanes = (size_t)c->num_cu * wf_waves(wf_options(c)) * 64u * (size_t)std::max(1, c->wf_pipes);
    CRT_ENSURE(c, c->w_overflow, lanes * wf_overflow_levels(c));
    return CRT_OK;
}

static int wf_ensure(crt_ctx *c, size_t P, size_t staging_elems, size_t list_elems, uint32_t ring)
{
    CRT_ENSURE(c, c->w_dead, list_elems / 8);   // dead-slot lists: one list's worth per pipe
    CRT_ENSURE(c, c->w_recA, list_elems);      // the ray records = the ray lists
    CRT_ENSURE(c, c->w_recB, list_elems);
    CRT_ENSURE(c, c->w_recC, list_elems);
    // (each array on its own: after a failed allocation that array reports n == 0 and is retried by the next call)
    CRT_ENSURE(c, c->w_ray_o, P);
    CRT_ENSURE(c, c->w_ray_d, P);
    CRT_ENSURE(c, c->w_sh_d, P);
    CRT_ENSURE(c, c->w_beta, P);
    CRT_ENSURE(c, c->w_radiance, P);
    CRT_ENSURE(c, c->w_nee, P);
    CRT_ENSURE(c, c->w_rng, P);
    CRT_ENSURE(c, c->w_misc, P);
    CRT_ENSURE(c, c->w_hit, P);
    CRT_ENSURE(c, c->w_vis, P);
    CRT_ENSURE(c, c->w_dflag, P);
    for (uint32_t b = 0; b < ring; b++)
        CRT_ENSURE(c, c->w_staging[b], staging_elems);
    CRT_ENSURE(c, c->w_tea, (size_t)c->tw * c->th);
    CRT_ENSURE(c, c->w_tile_cls, ((size_t)((c->tw + 7u) / 8u) * ((c->th + 7u) / 8u) + 15u) / 16u);
    if (!c->wf_host_ready) {
        if (!c->w_wq.p) {
            HIPCHK(c, c->w_wq.alloc(kWfRing));
            HIPCHK(c, hipMemset(c->w_wq.p, 0, kWfRing * sizeof(WfWorkQ)));
        }
        if (!c->ev_fork) HIPCHK(c, c->ev_fork.create(hipEventDisableTiming));
        if (!c->pub_stream) HIPCHK(c, c->pub_stream.create(hipStreamNonBlocking));
        for (int f = 0; f < crt_ctx::kFinishStreams; f++) {
            if (!c->fin_stream[f]) {
                int least = 0, greatest = 0;
                HIPCHK(c, hipDeviceGetStreamPriorityRange(&least, &greatest));
                HIPCHK(c, c->fin_stream[f].create(hipStreamNonBlocking, least));
            }
            if (!c->ev_fin[f]) HIPCHK(c, c->ev_fin[f].create(hipEventDisableTiming));
        }
        if (!c->h_dropped) HIPCHK(c, c->h_dropped.alloc(crt_ctx::kMaxPipes, hipHostMallocDefault));
        for (uint32_t b = 0; b < kWfRing; b++) {
            if (!c->ev_resolved[b]) HIPCHK(c, c->ev_resolved[b].create(hipEventDisableTiming));
            if (!c->ev_pub[b]) HIPCHK(c, c->ev_pub[b].create(hipEventDisableTiming));
        }
        for (int p = 0; p < crt_ctx::kMaxPipes; p++) {
            if (!c->w_ctl[p].p) {
                HIPCHK(c, c->w_ctl[p].alloc(1));
                HIPCHK(c, hipMemset(c->w_ctl[p].p, 0, sizeof(WfCtl)));
            }
            if (!c->h_status[p]) {
                // coherent pinned host memory that the shade kernel's first wave writes directly (write_status)
                HIPCHK(c, c->h_status[p].alloc(kStatusRing, hipHostMallocMapped | hipHostMallocCoherent));
                HIPCHK(c, hipHostGetDevicePointer((void **)&c->d_status[p], c->h_status[p].p, 0));
            }
            for (int k = 0; k < kStatusRing; k++) {
                if (!c->ev_status[p][k]) HIPCHK(c, c->ev_status[p][k].create(hipEventDisableTiming));
                if (!c->ev_done[p][k]) HIPCHK(c, c->ev_done[p][k].create(hipEventDisableTiming));
            }
            if (!c->ev_join[p]) HIPCHK(c, c->ev_join[p].create(hipEventDisableTiming));
            if (!c->ev_pub_join[p]) HIPCHK(c, c->ev_pub_join[p].create(hipEventDisableTiming));
            for (uint32_t b = 0; b < kWfRing; b++)
                if (!c->ev_evict[p][b]) HIPCHK(c, c->ev_evict[p][b].create(hipEventDisableTiming));
        }
        c->wf_host_ready = true;
    }
    return wf_ensure_overflow(c);
}

static int wf_resolve_batch(crt_ctx *c, const WfBatch &b)
{
    WfRun &r = *c->run;
    WfParams R = r.W[0];
    R.batch_id = b.id; R.n_samples = b.n;
    if (r.as.active) {                                           // adaptive: the active tiles only, no frame ring
        HIPCHK(c, wf_launch_resolve_adaptive(R, r.as, b.last_sample, c->stream));
        if (b.as_commit) HIPCHK(c, as_launch_commit(c->as_counts.p, r.as.active, r.as.n_active, b.as_commit, c->stream));
    } else {
        R.frames = c->d_frames.p; R.frame_ring = c->frame_ring;
        HIPCHK(c, wf_launch_resolve(R, b.last_sample, c->stream));
        c->resolved_upto = b.last_sample;
        if (c->frame_ring && c->frame_batch.size() == c->frame_ring)
            for (uint32_t k = 0; k < b.n && k < c->frame_ring; k++) c->frame_batch[(b.last_sample - 1u - k) % c->frame_ring] = (uint8_t)b.id;
    }
    HIPCHK(c, hipEventRecord(c->ev_resolved[b.id], c->stream));    // the id's queue, staging buffer and side pools are free after this
    r.resolved_recorded[b.id] = true;
    c->last_launches++;
    return CRT_OK;
}

// The host has seen the batch's queue reset complete: from here on launches may list the queue, and the status
// records of the iterations enqueued from here on describe THIS batch's queue (earlier ones may have looked at the
// cursors of the id's previous user).
static bool wf_check_ready(crt_ctx *c, WfBatch &b, bool wait)
{
    if (b.ready) return true;
    if (wait) { if (hipEventSynchronize(c->ev_pub[b.id]) != hipSuccess) return false; }
    else if (hipEventQuery(c->ev_pub[b.id]) != hipSuccess) return false;
    b.ready = true;
    for (int p = 0; p < c->run->K; p++) b.from_it[p] = c->run->pipes[p].it;
    return true;
}

// Which queues the next launches re-arm from: the open batches whose queue still holds work, oldest first.
static void wf_set_queues(crt_ctx *c, WfParams &W)
{
    WfRun &r = *c->run;
    uint32_t order[kWfRing], n = 0;
    for (WfBatch &b : r.open)
        if (wf_check_ready(c, b, false) && r.queue_left[b.id] && n < kWfRing) order[n++] = b.id;
    if (n == 0) order[n++] = r.open.empty() ? 0u : r.open.back().id;       // (all dry: any valid entry)
    for (uint32_t k = 0; k < kWfRing; k++) W.seg_order[k] = order[k < n ? k : n - 1];
    W.seg_n = n;
}

static int wf_retire_front(crt_ctx *c);
constexpr double kWfStallMs = 30000.0;     // a driver loop that makes no progress for this long gives up with CRT_EDEVICE

static bool wf_debug() { static const bool on = getenv("CRT_DEBUG") != nullptr; return on; }
double wf_now_ms()
{
    static const auto t_ref = std::chrono::steady_clock::now();
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_ref).count();
}


// Enqueue `iters` iterations of pipe p.  The shade launch of iteration i also writes iteration i - 1's status record.
static int wf_enqueue(crt_ctx *c, int p, uint32_t iters)
{
    WfRun &r = *c->run;
    WfPipeView &pp = r.pipes[p];
    WfParams &W = r.W[p];
    const hipStream_t stream = r.stream[p];
    if (pp.it - pp.it_confirmed + iters >= (uint32_t)kStatusRing || iters == 0) return fail(c, CRT_EDEVICE, "wavefront driver: status ring overrun");
    W.count_alive = r.open.size() > 1 ? 1u : 0u;
    wf_set_queues(c, W);
    const bool evicted = pp.evict_next != 0;
    for (uint32_t k = 0; k < iters; k++, pp.it++) {
        // Dead slots are listed by the shade launch and re-armed by a k_wf_gen launch behind it while a listed queue may
        // hold work (the host's view lags the device's: a launch too many finds the queues dry, a launch too few leaves
        // the slots dead for one more iteration).  (I11: a sweep of the whole pool behind a launch that deferred.)
        const WfLaunchMode mode = wf_launch_mode(pp, r.work_left, c->wf_defer_nee != 0);
        W.tail_bound = mode.tail_bound; W.rearm = mode.rearm; W.defer = mode.defer;
        W.evict_mask = pp.evict_next;
        W.status_out = pp.it > pp.it_first ? c->d_status[p] + (pp.it - 1u) % kStatusRing : nullptr;
        HIPCHK(c, wf_launch_shade(W, pp.it, stream));
        if (pp.it > pp.it_first) HIPCHK(c, hipEventRecord(c->ev_status[p][(pp.it - 1u) % kStatusRing], stream));   // (blocking waits fall back on it)
        pp.st_counted[pp.it % kStatusRing] = W.count_alive != 0;
        if (W.rearm) {
            HIPCHK(c, wf_launch_gen(W, pp.it, stream, r.as.active ? &r.as : nullptr));
            c->last_launches++;
            if (!r.as.active && wf_gen_mapped(W)) c->mapped_gen_launches++;
        }
        if (pp.evict_next) {                                     // k_wf_finish may start once this launch is through
            for (WfBatch &b : r.open)
                if ((pp.evict_next >> b.id) & 1u) {
                    HIPCHK(c, hipEventRecord(c->ev_evict[p][b.id], stream));
                    b.launched_mask |= 1u << p;
                }
            pp.evict_next = 0; W.evict_mask = 0;
        }
        if (c->time_kernels) {
            size_t need = 2 * (size_t)(c->last_trace_kernel_launches + 1);
            while (c->kev.size() < need) {
                Event e;
                HIPCHK(c, e.create());
                c->kev.push_back(std::move(e));
            }
            HIPCHK(c, hipEventRecord(c->kev[need - 2], stream));
        }
        HIPCHK(c, wf_launch_trace(W, pp.it, pp.blocks_now, stream));
        if (c->time_kernels) {
            HIPCHK(c, hipEventRecord(c->kev[2 * (size_t)c->last_trace_kernel_launches + 1], stream));
            c->last_trace_kernel_launches++;
        }
        HIPCHK(c, hipEventRecord(c->ev_done[p][pp.it % kStatusRing], stream));
        c->last_launches += 2;
        c->last_iterations++;
    }
    for (uint32_t k = 0; k < W.seg_n; k++) r.listed_until[W.seg_order[k]][p] = pp.it;
    return evicted && !r.all_evicting ? wf_retire_front(c) : CRT_OK;   // a batch may have become ready for its finish pass
}

// k_wf_finish for the leading batches whose evicting launches are all enqueued, then their resolve passes -- on
// the context's stream, which has nothing else to do while the pipes work.  One finish launch covers every pipe
// of every such batch: its duration is that of the longest path in it (one lane per path, a bounce after the
// other), so batches that are ready together cost one such tail, not one each.
static int wf_retire_front(crt_ctx *c)
{
    WfRun &r = *c->run;
    size_t n = 0;
    while (n < r.open.size() && r.open[n].evicting && (r.open[n].need_mask & ~r.open[n].launched_mask) == 0) n++;
    if (n == 0) return CRT_OK;
    // The finish launch goes to one of a few low-priority streams in turn (a launch lasts as long as its longest path,
    // a few milliseconds on S2 whatever the number of paths, so consecutive launches must overlap or the retirement
    // of small batches is bound by that latency); the resolve passes wait for it on the context's stream.
    const int f = c->fin_next;
    c->fin_next = (c->fin_next + 1) % crt_ctx::kFinishStreams;
    hipStream_t fs = c->fin_stream[f];
    WfFinishSegs G{};
    bool any = false;
    uint32_t bound = 1;                                         // paths per (batch, pipe) at most: alive slots only shrink once a queue is dry
    for (size_t i = 0; i < n; i++) bound = std::max(bound, r.open[i].evict_bound);
    auto launch = [&]() -> int {
        if (G.n == 0) return CRT_OK;
        WfParams F = r.W[0];
        F.tail_bound = c->wf_side_ppw;
        HIPCHK(c, wf_launch_finish(F, G, bound, fs));
        c->last_launches++;
        G.n = 0;
        any = true;
        return CRT_OK;
    };
    for (size_t i = 0; i < n; i++) {
        const WfBatch &b = r.open[i];
        for (int p = 0; p < r.K; p++) {
            if (!((b.need_mask >> p) & 1u)) continue;
            HIPCHK(c, hipStreamWaitEvent(fs, c->ev_evict[p][b.id], 0));
            if (G.n == kWfFinishSegs) CRT_TRY(launch());
            G.ctl[G.n] = r.W[p].ctl; G.base[G.n] = r.W[p].side_base[b.id]; G.batch[G.n] = b.id; G.n++;
        }
    }
    CRT_TRY(launch());
    if (any) {
        HIPCHK(c, hipEventRecord(c->ev_fin[f], fs));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_fin[f], 0));
    }
    for (size_t i = 0; i < n; i++) CRT_TRY(wf_resolve_batch(c, r.open[i]));   // in order
    r.open.erase(r.open.begin(), r.open.begin() + (long)n);
    return CRT_OK;
}

// Retirement after a status: decide the evictions (wf_decide_evictions), then finish and resolve what is ready.
static int wf_retire(crt_ctx *c)
{
    wf_decide_evictions(*c->run, wf_options(c));
    return wf_retire_front(c);
}

// One status record of pipe p has arrived: fold it into the driver's view.
static int wf_process_status(crt_ctx *c, int p)
{
    WfRun &r = *c->run;
    WfPipeView &pp = r.pipes[p];
    const int slot = (int)(pp.it_confirmed % kStatusRing);
    const WfStatus st = c->h_status[p].p[slot];                   // (the caller has seen it_end == it_confirmed + 1, with acquire)
    const bool counted = pp.st_counted[slot];
    if (st.it_end != pp.it_confirmed + 1u) return fail(c, CRT_EDEVICE, "wavefront driver: status record out of order (pipe %d: %u, expected %u)", p, st.it_end, pp.it_confirmed + 1u);
    if (st.dropped) return fail(c, CRT_EDEVICE, "wavefront pipeline: a capacity guard dropped %u paths (pipe %d)", st.dropped, p);
    wf_fold_status(r, p, st, counted);
    if (wf_debug()) {
        fprintf(stderr, "[crt  %8.2f] pipe %d it %u rays %llu open %zu work_left %d per_it %.0f alive", wf_now_ms(), p, st.it_end, st.rays, r.open.size(), (int)r.work_left, r.per_it);
        for (const WfBatch &b : r.open) fprintf(stderr, " %u:%u%s", b.id, pp.alive[b.id], b.evicting ? "e" : pp.dry[b.id] ? "d" : "");
        fprintf(stderr, "\n");
    }
    return wf_retire(c);
}

// Look at pipe p's oldest pending status record; block = wait for it.  *got says whether one was processed.
static int wf_poll(crt_ctx *c, int p, bool block, bool *got)
{
    WfPipeView &pp = c->run->pipes[p];
    if (got) *got = false;
    if (pp.it_confirmed >= pp.it) return CRT_OK;
    const uint32_t want = pp.it_confirmed + 1u;
    const int slot = (int)(pp.it_confirmed % kStatusRing);
    const uint32_t *flag = &c->h_status[p].p[slot].it_end;
    auto ready = [&]() { return __atomic_load_n(flag, __ATOMIC_ACQUIRE) == want; };
    if (!ready()) {
        if (!block) return CRT_OK;
        // the record is written by the NEXT iteration's shade launch: make sure there is one
        if (pp.it == want) CRT_TRY(wf_enqueue(c, p, 1));
        for (int spin = 0; spin < 2000 && !ready(); spin++) std::this_thread::yield();
        if (!ready()) {
            HIPCHK(c, hipEventSynchronize(c->ev_status[p][slot]));
            if (!ready()) return fail(c, CRT_EDEVICE, "wavefront driver: status record of pipe %d iteration %u did not arrive", p, want - 1u);
        }
    }
    if (got) *got = true;
    return wf_process_status(c, p);
}

static int wf_poll_all(crt_ctx *c)
{
    WfRun &r = *c->run;
    for (int p = 0; p < r.K; p++)
        for (;;) {
            bool got = false;
            CRT_TRY(wf_poll(c, p, false, &got));
            if (!got) break;
        }
    return CRT_OK;
}

// Block until some status arrives (enqueueing iterations first where nothing is in flight).
static int wf_wait_progress(crt_ctx *c)
{
    WfRun &r = *c->run;
    for (int p = 0; p < r.K; p++)
        if (!r.pipes[p].done && r.pipes[p].it - r.pipes[p].it_confirmed < 2u) CRT_TRY(wf_enqueue(c, p, r.pipes[p].chunk));
    for (int k = 0; k < r.K; k++) {
        const int p = (r.poll_next + k) % r.K;
        if (r.pipes[p].it == r.pipes[p].it_confirmed) continue;
        r.poll_next = (p + 1) % r.K;
        return wf_poll(c, p, true, nullptr);
    }
    return CRT_OK;
}

// Iterations of pipe p that are enqueued and have not completed.  (An iteration's status record only arrives with the
// NEXT iteration's shade launch, so a pipe that has run out of launches would look busy for ever by the records alone.)
static uint32_t wf_in_flight(crt_ctx *c, int p)
{
    WfPipeView &pp = c->run->pipes[p];
    if (pp.it_done < pp.it_confirmed) pp.it_done = pp.it_confirmed;
    while (pp.it_done < pp.it && hipEventQuery(c->ev_done[p][pp.it_done % kStatusRing]) == hipSuccess) pp.it_done++;
    return pp.it - pp.it_done;
}

// The driver's state in a line (for the error message of a loop that does not make progress).
std::string wf_state(crt_ctx *c)
{
    WfRun &r = *c->run;
    char buf[256];
    std::string out;
    snprintf(buf, sizeof buf, "K %d ring %u open %zu work_left %d per_it %.0f all_evicting %d |", r.K, r.ring, r.open.size(), (int)r.work_left, r.per_it, (int)r.all_evicting);
    out += buf;
    for (int p = 0; p < r.K; p++) {
        const WfPipeView &pp = r.pipes[p];
        snprintf(buf, sizeof buf, " pipe %d: it %u done %u confirmed %u rays %llu any %d finished %d evict %x |", p, pp.it, pp.it_done, pp.it_confirmed, pp.rays, (int)pp.any, (int)pp.done, pp.evict_next);
        out += buf;
    }
    size_t shown = 0;
    for (const WfBatch &b : r.open) {
        if (shown++ >= 3) break;
        snprintf(buf, sizeof buf, " batch %u: left %d ready %d evicting %d need %x launched %x", b.id, (int)r.queue_left[b.id], (int)b.ready, (int)b.evicting, b.need_mask, b.launched_mask);
        out += buf;
        for (int p = 0; p < r.K; p++) {
            snprintf(buf, sizeof buf, " [p%d alive %u valid %d dry %d from %u]", p, r.pipes[p].alive[b.id], (int)r.pipes[p].alive_valid[b.id], (int)r.pipes[p].dry[b.id], b.from_it[p]);
            out += buf;
        }
        out += ";";
    }
    return out;
}

// Is there room for another batch: a free batch id whose previous user's finish / resolve passes have COMPLETED (the
// new batch's queue reset waits for them on the device; a reset that waits stalls every pipe behind it).
static bool wf_has_room(crt_ctx *c)
{
    WfRun &r = *c->run;
    if (r.open.size() >= (size_t)r.ring) return false;
    const uint32_t id = r.open.empty() ? 0u : (r.open.back().id + 1u) % r.ring;
    if (!r.resolved_recorded[id]) return true;
    return hipEventQuery(c->ev_resolved[id]) == hipSuccess;
}

// ---- Invariants of the driver (publish / pump / retire), kept next to the loop that depends on all of them ----
//  I1  Iteration numbers of a pipe never repeat: a run starts 2 * kStatusRing behind the previous run's last number, so a
//      late status write of an earlier run can never match the `it_end` a poll is waiting for.
//  I2  Iteration i's status record is written by the FIRST wave of shade launch i + 1 (slot i % kStatusRing) and is
//      pending while it_confirmed <= i < it; wf_enqueue refuses to run more than kStatusRing - 1 ahead of it_confirmed, so
//      a slot is never rewritten before it has been read.  A poll accepts a slot only when its it_end is exactly
//      it_confirmed + 1 (acquire load of the word the device stores last, behind a system-scope fence).
//  I3  What a status says about a queue is FINAL for that launch: since round 3 nothing takes work inside a shade launch
//      (k_wf_gen does, between the shade launches), so cursors (`left`, `consumed`) and alive counts of one record are
//      one consistent cut -- taken after gen(i) has completed and before gen(i + 1) starts.
//  I4  A batch's statuses count only from launches enqueued after the HOST has seen its queue reset complete
//      (wf_check_ready sets from_it then; earlier launches may have read the id's previous extent).  Until then the
//      queue is not listed (wf_set_queues) and no launch can take its work.
//  I5  `dry[id]` of a pipe is monotone within a batch, and once a pipe has seen the queue dry no path of the batch can
//      start in that pipe any more (cursors only grow): alive[id] of that record bounds the pipe's paths from then on.
//      wf_retire evicts only when EVERY pipe's record says dry and the counts fit the side pools (k_wf_finish reports,
//      through WfCtl::dropped, if they did not).
//  I6  Batches resolve in publication order (the accumulator is summed in sample order); a batch id is reused only after
//      ev_resolved[id] of its previous user has COMPLETED (wf_has_room), and the reset of the id's queue additionally waits,
//      on the device, for launches that still list the old queue (listed_until) and for that resolve.
//  I7  Staging buffers, pool arrays and lists are never reallocated while r.live (wf_trace_batch flushes first).
//  I8  Every loop below makes progress or blocks on something the device will complete: a launch is always enqueued
//      behind the status being waited for (the record is written by the NEXT launch), back-pressure waits are on events
//      recorded behind enqueued work, and a wall-clock watchdog turns a violated assumption into CRT_EDEVICE + state dump.
//  I9  A flush returns with its finish / resolve passes still QUEUED on the context's stream (only crt_sync and the reads
//      wait for them).  Everything a new run starts is therefore ordered behind that stream: the pool's set-up runs on it,
//      the pipes AND the publishing stream wait for its fork event.  (I6's device-side waits are per run -- resolved_recorded
//      starts afresh -- so without the fork wait the reset of the new run's second batch could zero the side counters
//      under the previous run's k_wf_finish: round 3's lost-paths defect, test_flush_without_host_sync_then_quick_batches.)
//      WfCtl::dropped is never reset by a set-up, only once the host has reported it.
//  I10 Consumed work is not paths: k_wf_gen's CULL form decides whole work chunks itself -- it stores their
//      samples into the batch's staging buffer and starts nothing.  Nothing here assumes otherwise: `consumed` and `per_it`
//      only pace the feeding (a gen launch that culls takes MORE work per iteration; the estimate follows it), `alive`
//      counts what k_wf_gen started and k_wf_shade kept, and a pipe is drained when its queues are dry and it lists no rays
//      -- true from the first status on for a frame that is culled whole, whose queues drain inside gen launches alone
//      (while work is left every iteration re-lists the dead slots and launches k_wf_gen: rearm).  A batch is not resolved
//      before a culled sample's staging store has landed: the gen launch G that stored it took the work from the batch's
//      queue, so the queue was not dry before G; G belongs to some pipe p, and p's first status that says "dry" for the batch
//      is written by a shade launch BEHIND G in p's stream (a status written before G would have seen the work G took).  The
//      host resolves only after it has READ such a status from every pipe -- so G has completed, its stores with it, before
//      the resolve pass is even enqueued.  wf_retire asks every pipe that is not `done` for dry[b]; it skips a `done` pipe,
//      so wf_finish_all marks a pipe done only when that pipe's OWN records say dry for every open batch (r.work_left alone
//      may come from the other pipe's status, and a frame that is culled whole or nearly so lists no rays while its work
//      is still being taken, which without the cull practically never happened).  The batches still open when the flush
//      loop ends are resolved behind ev_join of every pipe.
//  I11 A deferred NEE entry (option "wf_defer_nee") stands where its slot stood.  Shade launch i of a pipe,
//      flagged `defer` (= rearm && wf_defer_nee), finishes a path that roulette ends with its shadow ray pending, frees
//      the slot and leaves an entry in nee[slot] / dflag[slot]; the slot's thread of launch i + 1 -- behind traversal launch
//      i in the stream -- stores the sample's final value iff the ray was visible and clears the entry.  The host sees
//      the timeline of the kWfDying route it replaces: the entry's shadow ray is in `rays` of iteration i and, where the
//      launch counts, the entry is in `alive[batch]` of iteration i; launch i + 1 adds nothing for it.  So whatever lets
//      the batch drain, be evicted or retire is a status of iteration i + 1 or later, which launch i + 2 writes -- the
//      host has READ it only when launch i + 1, and the fix-up store with it, has completed, before a finish or resolve
//      pass is enqueued (the argument of I10).  An evicting launch sweeps the pool (below), so it also consumes the
//      entries of the batches it evicts, ahead of the ev_evict it records for k_wf_finish and the resolve.
//      What makes this hold is that EVERY slot is visited by the launch behind one that deferred: tail mode visits only
//      the slots the ray lists name, and would miss an entry whose slot stayed dead or visit a re-armed slot twice
//      (through its camera-ray entry and through the old shadow entry).  Hence the rule: a pipe's launch is a pool sweep
//      whenever its previous launch had `defer` on, whatever pp.tail_bound says (wf_launch_mode, crt_wf_policy.h, which
//      alone keeps pp.last_defer).  Tail mode is chosen only when no work is left, when rearm and with it defer are off:
//      the sweep is one launch per run end at most, it creates no entry itself, and tail mode starts with the launch
//      after it.  The flush's final evicting launch obeys the same rule, so no entry outlives a run; k_wf_init clears
//      the flags of a pool that is set up afresh (a run abandoned after an error may have left some).
//
// Feed the pool: enqueue the iterations the published work needs (see the head of this section).  for_room = false:
// return once they are enqueued (the call does not wait for its work); for_room = true: keep feeding and reading
// statuses until there is room for another batch (back-pressure of a caller that publishes faster than the pool works).
static int wf_pump(crt_ctx *c, bool for_room)
{
    WfRun &r = *c->run;
    const WfOptions o = wf_options(c);
    const uint32_t max_ahead = (uint32_t)std::max(c->wf_ahead, c->wf_chunk + 1);   // iterations in flight per pipe before the driver waits
    const double t_start = wf_now_ms();
    for (int guard = 0; guard < 4000000; guard++) {
        if ((guard & 63) == 63 && wf_now_ms() - t_start > kWfStallMs) return fail(c, CRT_EDEVICE, "wavefront driver: pump stalled (%s)", wf_state(c).c_str());
        CRT_TRY(wf_poll_all(c));
        if (for_room && wf_has_room(c)) return CRT_OK;
        unsigned long long inflight = 0;
        uint32_t fl[crt_ctx::kMaxPipes];
        for (int p = 0; p < r.K; p++) { fl[p] = wf_in_flight(c, p); inflight += fl[p]; }
        const WfFeed feed = wf_feed(r, o, inflight);
        const double need = feed.need;
        if (!(need > 0.0)) {
            if (!for_room) return CRT_OK;
            // nothing to feed, but the oldest batch has yet to retire: its last paths need iterations (or only its
            // finish / resolve passes are still running on the device)
            if (wf_debug()) fprintf(stderr, "[pump %8.2f] no room and nothing to feed (open %zu)\n", wf_now_ms(), r.open.size());
            if (r.open.size() < (size_t)r.ring) {
                const uint32_t id = (r.open.back().id + 1u) % r.ring;
                HIPCHK(c, hipEventSynchronize(c->ev_resolved[id]));
                r.resolved_recorded[id] = false;                 // (complete: nothing to wait for any more)
                continue;
            }
            CRT_TRY(wf_wait_progress(c));
            continue;
        }
        // the pipe with the fewest iterations in flight takes the next chunk
        int p = 0;
        for (int q = 1; q < r.K; q++) if (fl[q] < fl[p]) p = q;
        WfPipeView &pp = r.pipes[p];
        if (pp.it - pp.it_confirmed + (uint32_t)c->wf_chunk >= (uint32_t)kStatusRing - 1u) {
            CRT_TRY(wf_poll(c, p, true, nullptr));              // (out of status slots: wait for this pipe's oldest record)
            continue;
        }
        if (fl[p] >= max_ahead) {                                // back-pressure: wait for this pipe's oldest iteration
            const double t0 = wf_debug() ? wf_now_ms() : 0.0;
            HIPCHK(c, hipEventSynchronize(c->ev_done[p][pp.it_done % kStatusRing]));
            pp.it_done++;                                        // (known now, whatever a later hipEventQuery says)
            if (wf_debug()) fprintf(stderr, "[pump %8.2f] waited %.2f ms for pipe %d (in flight %u %u, need %.0f, room %d)\n", wf_now_ms(), wf_now_ms() - t0, p, fl[0], fl[r.K - 1], need, (int)for_room);
            continue;
        }
        // (a batch whose queue reset has not been seen complete is not listed yet: wait for it rather than launch
        // iterations that cannot take its work)
        {
            bool listed = false;
            WfBatch *pending = nullptr;
            for (WfBatch &b : r.open) {
                if (!r.queue_left[b.id]) continue;
                if (wf_check_ready(c, b, false)) listed = true; else if (!pending) pending = &b;
            }
            if (!listed && pending && !wf_check_ready(c, *pending, true)) return fail(c, CRT_EDEVICE, "wavefront driver: queue reset failed");
        }
        const uint32_t iters = wf_feed_iters(r, o, feed);
        const double t0 = wf_debug() ? wf_now_ms() : 0.0;
        CRT_TRY(wf_enqueue(c, p, iters));
        if (wf_debug()) fprintf(stderr, "[pump %8.2f] enqueued %u on pipe %d in %.3f ms (in flight %u %u, need %.0f, open %zu)\n", wf_now_ms(), iters, p, wf_now_ms() - t0, fl[0], fl[r.K - 1], need, r.open.size());
    }
    return fail(c, CRT_EDEVICE, "wavefront driver: pump did not converge");
}

// A cheap turn of the driver for calls that publish nothing themselves (a small call that is only noted, a query of the
// latest frame): read the statuses that have arrived, and where a retirement decision waits for a pipe's next shade launch
// (evict_next), give it one -- so that batches keep retiring (finish + resolve) while a display loop runs ahead of them.
int wf_tick(crt_ctx *c)
{
    if (!c->run || !c->run->live || c->in_publish) return CRT_OK;
    WfRun &r = *c->run;
    CRT_TRY(wf_poll_all(c));
    for (int p = 0; p < r.K; p++) {
        WfPipeView &pp = r.pipes[p];
        if (pp.evict_next == 0 || pp.done) continue;
        if (wf_in_flight(c, p) >= (uint32_t)std::max(c->wf_ahead, c->wf_chunk + 1)) continue;
        if (pp.it - pp.it_confirmed + 1u >= (uint32_t)kStatusRing - 1u) continue;
        CRT_TRY(wf_enqueue(c, p, 1));
    }
    return CRT_OK;
}

// Run everything in the pool to its end and resolve every batch.
static int wf_finish_all(crt_ctx *c)
{
    WfRun &r = *c->run;
    const int K = r.K;
    const WfOptions o = wf_options(c);
    const unsigned long long flush_at = wf_flush_at(o);
    for (int p = 0; p < K; p++) { r.pipes[p].done = false; r.pipes[p].chunk = (uint32_t)c->wf_chunk; }
    for (WfBatch &b : r.open) if (!wf_check_ready(c, b, true)) return fail(c, CRT_EDEVICE, "wavefront driver: queue reset failed");
    r.all_evicting = false;
    int active = K;
    const double t_start = wf_now_ms();
    for (unsigned long long guard = 0; active > 0; guard++) {
        if (guard > 4000000ull || ((guard & 15) == 15 && wf_now_ms() - t_start > 4.0 * kWfStallMs))
            return fail(c, CRT_EDEVICE, "wavefront pipeline did not drain (%s)", wf_state(c).c_str());
        // one chunk is always enqueued AHEAD of the status being waited for, so the GPU never idles on the host
        // (iteration i's status record is written by the launch of iteration i + 1: three in flight = one ahead of the
        // one whose record is being waited for)
        for (int p = 0; p < K; p++)
            while (!r.pipes[p].done && r.pipes[p].it - r.pipes[p].it_confirmed < 3u) CRT_TRY(wf_enqueue(c, p, 1));
        int p = -1;
        for (int k = 0; k < K && p < 0; k++) {
            const int q = (r.poll_next + k) % K;
            if (!r.pipes[q].done && r.pipes[q].it > r.pipes[q].it_confirmed) p = q;
        }
        if (p < 0) break;
        r.poll_next = (p + 1) % K;
        CRT_TRY(wf_poll(c, p, true, nullptr));
        WfPipeView &pp = r.pipes[p];
        // chunks shrink as the queues run dry: what is enqueued ahead of the status that shows them empty runs on a
        // nearly empty pool, and the host needs only ~20 us per launch to keep up
        if (!r.work_left) pp.chunk = 1;
        if (wf_pipe_drained(r, p)) { pp.done = true; active--; continue; }
        (void)wf_tail_walk(r, o, p);
        if (wf_flush_all_ready(r, o)) {
            const uint32_t mask = wf_open_mask(r);
            for (int q = 0; q < K; q++) {
                WfPipeView &pq = r.pipes[q];
                if (pq.done) continue;
                pq.evict_next = mask;
                CRT_TRY(wf_enqueue(c, q, 1));                     // one more iteration: its shade launch empties the pool
                pq.done = true; pq.rays = 0;
            }
            active = 0;
            r.all_evicting = true;
        }
    }
    // everything enqueued for the pipes comes before the finish / resolve passes on the context's stream
    for (int p = 0; p < K; p++) {
        HIPCHK(c, hipEventRecord(c->ev_join[p], r.stream[p]));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_join[p], 0));
    }
    while (!r.open.empty()) {                                    // in order: the accumulator is summed in sample order
        const WfBatch &b = r.open.front();
        if (r.all_evicting || b.evicting) {
            // (nothing else is running: few paths per wave end sooner)
            WfFinishSegs G{};
            for (int p = 0; p < K; p++) { G.ctl[G.n] = r.W[p].ctl; G.base[G.n] = r.W[p].side_base[b.id]; G.batch[G.n] = b.id; G.n++; }
            WfParams F = r.W[0];
            F.tail_bound = c->wf_flush_ppw;
            // (a batch whose eviction began before the final one may hold up to a side pool's worth)
            HIPCHK(c, wf_launch_finish(F, G, (uint32_t)std::max<unsigned long long>(std::max<unsigned long long>(flush_at, 1), b.evicting ? b.evict_bound : 0u), c->stream));
            c->last_launches++;
        }
        CRT_TRY(wf_resolve_batch(c, b));
        r.open.erase(r.open.begin());
    }
    // (the status records still pending describe an empty pool; the capacity guards are checked below)
    for (int p = 0; p < K; p++) r.pipes[p].it_confirmed = r.pipes[p].it;
    // The pipes' sharded counters, summed, taken off the device and zeroed there: counters 0..CRT_NCOUNTERS-1 go to `tot`
    // (where given), the shade kernel's phase clocks and the traversal probes (8..15) to crt_debug_probes.
    auto fold_counters = [&](unsigned long long *tot) -> int {
        for (int p = 0; p < K; p++) {
            unsigned long long sh[kWfShards][CRT_NCOUNTERS_DEV], pc[CRT_NCOUNTERS_DEV];
            HIPCHK(c, hipMemcpy(sh, &c->w_ctl[p].p->counters[0][0], sizeof sh, hipMemcpyDeviceToHost));
            for (int k = 0; k < CRT_NCOUNTERS_DEV; k++) { pc[k] = 0; for (uint32_t s_ = 0; s_ < kWfShards; s_++) pc[k] += sh[s_][k]; }
            for (int k = 0; tot && k < CRT_NCOUNTERS; k++) tot[k] += pc[k];
            for (int k = 0; k < 8; k++) c->probes[k] += pc[8 + k];
            HIPCHK(c, hipMemset(&c->w_ctl[p].p->counters[0][0], 0, sizeof(unsigned long long) * CRT_NCOUNTERS_DEV * kWfShards));
        }
        return CRT_OK;
    };
#ifdef CRT_WF_PROBE
    if (!c->counting) {                                          // probe build: the phase clocks alone
        HIPCHK(c, hipStreamSynchronize(c->stream));
        CRT_TRY(fold_counters(nullptr));
    }
#endif
    if (c->counting) {
        // fold the pipes' counters into the context's
        HIPCHK(c, hipStreamSynchronize(c->stream));
        unsigned long long tot[CRT_NCOUNTERS];
        HIPCHK(c, hipMemcpy(tot, c->d_counters.p, sizeof tot, hipMemcpyDeviceToHost));
        CRT_TRY(fold_counters(tot));
        HIPCHK(c, hipMemcpy(c->d_counters.p, tot, sizeof tot, hipMemcpyHostToDevice));
    }
    // (checked by wf_check_dropped after the caller's stream synchronisation: k_wf_finish's guard)
    for (int p = 0; p < K; p++)
        HIPCHK(c, hipMemcpyAsync(&c->h_dropped.p[p], &c->w_ctl[p].p->dropped, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    // the pool is empty; the next batch sets the pipes up afresh
    r.live = false;
    return CRT_OK;
}

// After a flush and a synchronisation of the context's stream: did a device-side capacity guard drop a path?
int wf_check_dropped(crt_ctx *c)
{
    if (!c->h_dropped) return CRT_OK;
    for (int p = 0; p < crt_ctx::kMaxPipes; p++)
        if (c->h_dropped.p[p]) {
            const uint32_t n = c->h_dropped.p[p];
            c->h_dropped.p[p] = 0;
            // (the device counter is not reset by the pool's set-up -- a flush in the middle of a run must not lose what an
            // earlier one counted -- but here, once reported)
            if (c->w_ctl[p].p) (void)hipMemsetAsync(&c->w_ctl[p].p->dropped, 0, sizeof(uint32_t), c->stream);
            return fail(c, CRT_EDEVICE, "wavefront pipeline: a capacity guard dropped %u paths (pipe %d); the frame is incomplete", n, p);
        }
    return CRT_OK;
}

// Turn the samples requested by crt_trace into batches.  Small calls are merged (option "wf_cohort", 16 samples):
// the shards of a batch's work queue are its samples, which sweep the frame together, so the paths in flight at any
// time all start inside one band of the image, many samples deep -- and the rays of a launch touch a slice of the
// scene instead of all of it (a batch of one sample per pixel has four whole frames in flight and
// costs 1.5x as much per sample).  force: publish whatever is pending (crt_sync and every call that reads state).
int wf_publish_pending(crt_ctx *c, bool force)
{
    if (c->in_publish) return CRT_OK;
    const bool defer = c->wf_defer && !c->counting;
    const WfOptions o = wf_options(c);
    const uint32_t cap = wf_batch_cap(o), cohort = wf_cohort_size(o, cap);
    c->in_publish = true;
    int rc = CRT_OK;
    while (c->pending > 0 && rc == CRT_OK) {
        const uint32_t take = std::min(c->pending, cap);
        if (take < cap && !force && defer && take < cohort) break;      // wait for more calls
        c->pending -= take;
        const uint32_t published0 = c->published;
        rc = wf_trace_batch(c, take);
        if (rc != CRT_OK) {                                       // what could not be published never happened
            c->sample -= take + c->pending;
            c->pending = 0;
            c->published = published0;                            // (a failure behind `published += n` drained the pool: those samples are gone too)
        }
    }
    c->in_publish = false;
    return rc;
}

// A failed drive leaves the pool in an unknown state: drain the streams and start afresh next time.
static void wf_abandon(crt_ctx *c)
{
    for (const Stream &s : c->pipe_stream) s.sync();
    (void)hipStreamSynchronize(c->stream);
    c->run->live = false;
    c->run->open.clear();
}

// Finish whatever the pipeline still holds (no-op when nothing is in flight).
int wf_flush(crt_ctx *c)
{
    if (c->pending || (c->run && c->run->live)) HIPCHK(c, hipSetDevice(c->device));   // (publishing allocates and launches)
    if (c->pending && !c->in_publish && c->pipeline == 1 && c->accel_mode == CRT_ACCEL_BVH2) CRT_TRY(wf_publish_pending(c, true));
    if (!c->run || !c->run->live) return CRT_OK;
    int rc = wf_finish_all(c);
    if (rc != CRT_OK) { wf_abandon(c); return rc; }
    if (c->last_timed) HIPCHK(c, hipEventRecord(c->ev1, c->stream));   // crt_last_trace_ms covers the stragglers too
    return rc;
}

// One batch of n samples through the wavefront pipeline.  as: a batch of the active tiles of an adaptive call -- its queue
// holds n * n_active * 64 work ids; the pool is sized as for the uniform batch of n samples, so that rounds with fewer
// active tiles neither shrink nor reallocate it.
int wf_trace_batch(crt_ctx *c, uint32_t n, const AsBatch *as)
{
    if (!c->run) c->run.reset(new WfRun());
    WfRun &r = *c->run;
    const WfOptions o = wf_options(c);
    const WfConfig g = wf_config(o, n);
    if (g.npix == 0 || n == 0) { int rc = wf_flush(c); if (!as) c->published += n; return rc; }
    unsigned long long work_total = g.work_total;
    uint32_t work_per_shard = g.work_per_shard;
    // region-major shards (option "wf_affinity", read here: DESIGN.md 5.11); the adaptive queues keep the plain ranges
    const uint32_t map_samples = as ? 0u : g.map_samples;
    if (as) {
        work_total = (unsigned long long)n * as->n_active * 64u;
        work_per_shard = (uint32_t)(((work_total + kWfShards - 1) / kWfShards + 63u) & ~63ull);
    }
    // (adaptive: + the tile's count, in k_wf_gen.  The sample offset moves the RNG / stratum index alone: work ids, the
    // staging layout and last_sample, which the resolve pass tone-maps with and indexes the frame ring by, count from the reset)
    // (adaptive: the offset is 0 unless option "adaptive_temporal" let it in)
    const uint32_t first_sample = as ? c->sample_offset + as->off + 1u : c->sample_offset + c->published + 1u;
    const uint32_t last_sample = as ? as->off + n : c->published + n;
    // counting folds counters on the host after every batch; otherwise batches are pipelined across calls
    const bool defer = c->wf_defer && !c->counting;
    const size_t staging_elems = (size_t)n * g.npix;
    const uint32_t side_slots = kWfRing * (uint32_t)crt_ctx::kMaxPipes * kWfSideCap;   // side pools first, then the pool
    // (a live pool is kept unless the batch needs another: wf_must_restart)
    if (r.live) {
        size_t staging_min = (size_t)-1;
        for (uint32_t b = 0; b < r.ring; b++) staging_min = std::min(staging_min, c->w_staging[b].n);
        const bool other_kind = (r.as.active != nullptr) != (as != nullptr) || (as && r.as.n_active != as->n_active);
        if (wf_must_restart(r, g.P, staging_elems, staging_min, other_kind)) CRT_TRY(wf_flush(c));
    }
    const uint32_t pool_slots = r.live ? r.P : g.P;
    const size_t list_elems = r.live ? (size_t)8 * r.list_cap * kWfShards * (size_t)r.K : g.list_per_pipe * (size_t)g.K;
    if (!r.live) r.ring = wf_ring_size(o, staging_elems);
    CRT_TRY(wf_ensure(c, (size_t)pool_slots + side_slots, staging_elems, list_elems, r.ring));
    if (!r.live) {
        r.K = g.K; r.P = g.P; r.Pp = g.Pp; r.list_cap = g.list_cap;
        r.trace_blocks = wf_trace_blocks(o, c->num_cu);
        r.open.clear();
        WfBatch nb;
        nb.n = n; nb.last_sample = last_sample; nb.id = 0; nb.as_commit = as ? as->commit : 0u;
        r.open.push_back(nb);
        r.seg_total[0] = work_total; r.seg_wps[0] = work_per_shard;
        for (uint32_t b = 0; b < kWfRing; b++) {
            r.queue_left[b] = false; r.consumed[b] = 0; r.resolved_recorded[b] = false;
            for (int p = 0; p < crt_ctx::kMaxPipes; p++) r.listed_until[b][p] = 0;
        }
        r.queue_left[0] = r.work_left = true;
        r.consumed_total = 0; r.rate_consumed = 0; r.rate_its = 0;                // (rate_its: set below, once the pipes' iteration numbers are)
        r.per_it = (double)g.Pp;                                 // an empty pool takes a slot's worth per slot
        r.all_evicting = false; r.poll_next = 0;
        r.as = as ? AsTiles{c->as_active.p, c->as_counts.p, c->as_q.p, as->n_active} : AsTiles{};
        for (int p = 0; p < r.K; p++) {
            const uint32_t it0 = r.pipes[p].it + 2u * (uint32_t)kStatusRing;
            r.pipes[p] = WfPipeView();
            r.W[p] = WfParams{};
            r.pipes[p].it = r.pipes[p].it_first = r.pipes[p].it_confirmed = r.pipes[p].it_done = it0;
            r.pipes[p].chunk = (uint32_t)c->wf_chunk;
            WfParams &W = r.W[p];
            W.sc = c->sc;
            W.ray_o = c->w_ray_o.p; W.ray_d = c->w_ray_d.p; W.sh_d = c->w_sh_d.p; W.beta = c->w_beta.p;
            W.radiance = c->w_radiance.p; W.nee = c->w_nee.p; W.rng = c->w_rng.p; W.misc = c->w_misc.p;
            W.hit = c->w_hit.p; W.vis = c->w_vis.p; W.dflag = c->w_dflag.p;
            W.dead = c->w_dead.p + (g.list_per_pipe / 8) * (size_t)p;
            W.rearm = 0; W.defer = 0;
            W.gen_blocks = wf_gen_blocks(o, g.list_cap);
            W.cull_miss = c->wf_cull_miss ? 1u : 0u;
            W.recA = c->w_recA.p + g.list_per_pipe * (size_t)p; W.recB = c->w_recB.p + g.list_per_pipe * (size_t)p;
            W.recC = c->w_recC.p + g.list_per_pipe * (size_t)p;
            for (uint32_t b = 0; b < kWfRing; b++) {
                W.staging[b] = c->w_staging[b < r.ring ? b : 0].p;
                W.side_base[b] = (b * (uint32_t)crt_ctx::kMaxPipes + (uint32_t)p) * kWfSideCap;
                W.seg[b] = WfSeg{0, 64, 0, 0, 0};
                W.seg_order[b] = 0;
            }
            W.batch_id = 0; W.count_alive = 0; W.keep_pool = 0; W.evict_mask = 0; W.status_out = nullptr;
            W.ctl = c->w_ctl[p].p; W.wq = c->w_wq.p;
            W.slot_base = side_slots + g.Pp * (uint32_t)p; W.reset_wq = (p == 0) ? 1u : 0u;
            W.P = g.Pp; W.x0 = c->x0; W.y0 = c->y0; W.tw = c->tw; W.th = c->th;
            W.band = c->band; W.stride = c->stride; W.phase = c->phase;
            W.tiles_x = g.tiles_x; W.tiles_y = g.tiles_y; W.npix_padded = g.npix_padded;
            W.list_cap = g.list_cap;
            W.seg[0] = WfSeg{work_total, work_per_shard, first_sample, map_samples, 0u};
            W.affinity = map_samples ? 1u : 0u;
            W.seg_n = 1;
            W.n_samples = n;
            W.accum = accum_ptr(c); W.rgba = rgba_ptr(c);
            W.tea = c->w_tea.p;
            W.count = c->counting ? 1u : 0u;
            W.overflow_lanes = (uint32_t)c->num_cu * wf_waves(o) * 64u;
            W.stack_overflow = c->w_overflow.p + (size_t)p * W.overflow_lanes * wf_overflow_levels(c);
            W.trace_form = (uint32_t)c->wf_trace_form;
            // the tile classes: where k_wf_gen takes its CULL form.  They are this run's: every call that
            // changes what they depend on (camera, frame, tile rectangle and row mapping, the tree) ends the run first.
            W.tile_cls = (!as && c->wf_cull_classes && wf_gen_culls(W)) ? c->w_tile_cls.p : nullptr;
            W.cls_miss_zero = c->cie_zero ? 1u : 0u;
            if (!c->pipe_stream[p]) {
                // Streams beyond the hardware queues (4 by default) share one, and two pipes sharing a queue do not
                // overlap at all (measured: 95 instead of 77 ms per S2 frame when the caller's framework had taken
                // the queues first).  The runtime keeps separate queues per priority level and frameworks create
                // their stream pools at the default level, so the pipes take the high one -- all of them the same,
                // an uneven pair measured 4-9 % slower.
                int least = 0, greatest = 0;
                HIPCHK(c, hipDeviceGetStreamPriorityRange(&least, &greatest));
                HIPCHK(c, c->pipe_stream[p].create(hipStreamNonBlocking, greatest));
            }
            r.stream[p] = c->pipe_stream[p];
            r.pipes[p].blocks_now = r.trace_blocks;
        }
        for (int p = 0; p < r.K; p++) r.rate_its += r.pipes[p].it_confirmed;
        // The context's stream sets the pool up and forks the pipes (and, later, finishes stragglers and
        // resolves).  The pipes run on their own streams.
        HIPCHK(c, wf_launch_init(r.W[0], c->stream));
        HIPCHK(c, wf_launch_tea(r.W[0], c->w_tea.p, c->stream));          // per-pixel RNG seed words of this tile
        if (r.W[0].tile_cls) { HIPCHK(c, wf_launch_tile_classes(r.W[0], c->w_tile_cls.p, c->stream)); c->tile_cls_setups++; }
        HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));
        for (int p = 0; p < r.K; p++) {
            HIPCHK(c, hipStreamWaitEvent(r.stream[p], c->ev_fork, 0));
            if (p > 0) HIPCHK(c, wf_launch_init(r.W[p], r.stream[p]));
        }
        // The publishing stream too: the finish / resolve passes of the PREVIOUS run may still be queued on the context's
        // stream (a flush returns without waiting for them), and the queue / side-counter reset of this run's second batch
        // must not overtake them -- resolved_recorded, which orders that reset within a run, starts afresh here.  (A reset
        // that did: k_wf_finish found side_count 0 and the batch lost its last paths -- tests: display state machine walk.)
        HIPCHK(c, hipStreamWaitEvent(c->pub_stream, c->ev_fork, 0));
        r.live = true;
    } else {
        // room in the ring first (back-pressure: the oldest batch has to retire; the pool is fed meanwhile)
        CRT_TRY(wf_pump(c, true));
        // The batches in flight keep their slots, queues and staging buffers; this one takes the next id and its
        // work flows into the slots that are free once the older queues are dry.
        WfBatch nb;
        nb.n = n; nb.last_sample = last_sample; nb.id = (r.open.back().id + 1u) % r.ring; nb.as_commit = as ? as->commit : 0u;
        const uint32_t id = nb.id;
        r.seg_total[id] = work_total; r.seg_wps[id] = work_per_shard;
        r.queue_left[id] = r.work_left = true;
        r.consumed[id] = 0;
        for (int p = 0; p < r.K; p++) {
            WfPipeView &pp = r.pipes[p];
            WfParams &W = r.W[p];
            nb.from_it[p] = 0xFFFFFFFFu;                         // (set when the host sees the queue reset complete: wf_check_ready)
            W.seg[id] = WfSeg{work_total, work_per_shard, first_sample, map_samples, 0u};
            W.affinity = map_samples ? 1u : 0u;                  // (the traversal waves follow the newest batch's setting)
            W.n_samples = n;
            W.batch_id = id; W.keep_pool = 1;
            pp.tail_bound = 0; pp.blocks_now = r.trace_blocks;
            pp.any = false; pp.chunk = (uint32_t)c->wf_chunk; pp.done = false;
            pp.dry[id] = false; pp.alive_valid[id] = false; pp.alive[id] = 0;
        }
        // This batch's queue and side counters are reset on a stream of their own, which waits only for what it must:
        // a launch still in flight that has the id's OLD queue in its list (enqueued while that held work; it would
        // take the new work with the old batch's parameters), and the finish / resolve passes of the batch that
        // used the id before (they read its side pools and staging buffer).  No pipe waits for the reset: the queue is
        // listed by the launches that are enqueued after the host has seen the reset complete.
        for (int p = 0; p < r.K; p++)
            if (r.listed_until[id][p] > r.pipes[p].it_confirmed) {
                HIPCHK(c, hipEventRecord(c->ev_pub_join[p], r.stream[p]));
                HIPCHK(c, hipStreamWaitEvent(c->pub_stream, c->ev_pub_join[p], 0));
            }
        if (r.resolved_recorded[id]) HIPCHK(c, hipStreamWaitEvent(c->pub_stream, c->ev_resolved[id], 0));
        for (int p = 0; p < r.K; p++) HIPCHK(c, wf_launch_init(r.W[p], c->pub_stream));   // (one block each)
        HIPCHK(c, hipEventRecord(c->ev_pub[id], c->pub_stream));
        nb.ready = false;                                        // listed by the launches enqueued once the host has seen that event complete
        r.open.push_back(nb);
    }
    if (!as) c->published += n;
    int rc = wf_pump(c, false);
    if (rc == CRT_OK && !defer) rc = wf_flush(c);
    if (rc != CRT_OK && r.live) wf_abandon(c);
    return rc;
}

// Drive the pipeline until the resolve pass of the batch that holds `sample` is on the context's stream.
int wf_wait_sample(crt_ctx *c, uint32_t sample)
{
    if (sample <= c->resolved_upto) return CRT_OK;
    if (c->pipeline != 1 || c->accel_mode != CRT_ACCEL_BVH2) return wf_flush(c);
    if (sample > c->published) CRT_TRY(wf_publish_pending(c, true));   // (merged small calls wait for more: not any longer)
    const double t_start = wf_now_ms();
    for (int guard = 0; sample > c->resolved_upto; guard++) {
        WfRun *r = c->run.get();
        if (!r || !r->live || r->open.empty()) break;
        // the newest batch is only retired by a flush (nothing comes behind it under which its tail could finish)
        if (r->open.back().last_sample - r->open.back().n < sample) return wf_flush(c);
        if ((guard & 15) == 15 && wf_now_ms() - t_start > kWfStallMs) return fail(c, CRT_EDEVICE, "wavefront driver: waiting for sample %u stalled (%s)", sample, wf_state(c).c_str());
        CRT_TRY(wf_poll_all(c));
        if (sample <= c->resolved_upto) break;
        CRT_TRY(wf_wait_progress(c));
    }
    return CRT_OK;
}

}  // namespace crt
