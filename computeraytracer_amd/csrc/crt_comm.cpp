// crt_comm.cpp -- the multi-GPU part of the C ABI (include/crt.h, "Multi-GPU"): the frame partitioned by rows across the
// ranks of a communicator, one context per GPU, and the path's ONE exchange step -- the gather of the finished strips --
// as an RCCL all-gather over xGMI issued from libcrt itself, so that any host above the C ABI (the Node addon as much as
// the Python one) reaches the multi-GPU configurations.  The reference has a single GPUDevice (src/main.js:8-9) and no
// exchange of any kind; SURVEY 8(e) defines this one.
//
// Written against the public C ABI only (crt_set_row_bands / crt_set_tile, crt_bind_output, crt_get_stream): a context
// does not know that it is part of a communicator, it renders its rows into the strip buffers bound here.  Whether it
// still does is asked of it the same way (crt_device_buffers, crt_image_size, crt_tile: `current` below).  The one thing
// the public ABI does not show -- the frame state that CRT_GATHER_PREVIEW ships and records (uniform or adaptive, the sample
// count, the epoch, the adaptive state's Q and tile counts) -- comes through crt_internal_frame_state; the frame-level
// filters of crt_denoise_api.cpp ask for the assembled planes through crt_internal_comm_frame_view.
//
// Transports behind one interface:
//   RCCL   one process per GPU (or one thread per GPU): ncclCommInitRank + ncclAllGather.  librccl is loaded on first
//          use (dlopen), so single-GPU hosts never pay for it.
//   local  contexts of ONE process (any devices, the same one included): every rank copies its strip into every rank's
//          gather buffer with hipMemcpyPeerAsync and the ranks' streams are joined by events.  What one process driving
//          several GPUs uses, and what lets the partition / gather / assembly path be tested on a one-GPU box.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <dlfcn.h>

#include <atomic>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/crt.h"

namespace crt {
hipError_t launch_assemble(const void *full, void *frame, uint32_t elem_bytes, uint32_t W, uint32_t H, uint32_t world, uint32_t rows_max,
                           uint32_t band, hipStream_t stream);
}
extern "C" int crt_internal_fail(crt_ctx *c, int code, const char *msg);
// crt_api.cpp: out[3] = state (0 uniform, 1 adaptive), uniform sample count, epoch of the frame state; with `finish` a sync
// point first; q_dev / counts_dev: the adaptive state's device buffers
extern "C" int crt_internal_frame_state(crt_ctx *c, int finish, const char *who, uint32_t out[3], void **q_dev, void **counts_dev);

namespace {

// ---------------------------------------------------------------- RCCL, loaded on demand
struct Rccl {
    void *lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    std::string err;
    bool load()
    {
        if (lib) return true;
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (lib) break;
        }
        if (!lib) { err = std::string("librccl could not be loaded: ") + dlerror(); return false; }
        GetUniqueId = (decltype(GetUniqueId))dlsym(lib, "ncclGetUniqueId");
        CommInitRank = (decltype(CommInitRank))dlsym(lib, "ncclCommInitRank");
        AllGather = (decltype(AllGather))dlsym(lib, "ncclAllGather");
        CommDestroy = (decltype(CommDestroy))dlsym(lib, "ncclCommDestroy");
        GetErrorString = (decltype(GetErrorString))dlsym(lib, "ncclGetErrorString");
        if (!GetUniqueId || !CommInitRank || !AllGather || !CommDestroy || !GetErrorString) {
            err = "librccl lacks an expected entry point";
            dlclose(lib); lib = nullptr;
            return false;
        }
        return true;
    }
};
Rccl g_rccl;
std::mutex g_mu;                                   // guards g_rccl, g_comms and g_groups (never held across a GPU wait)

// ---------------------------------------------------------------- the local transport's shared state
struct Comm;
// The gathered planes.  Each is a row partition of a small frame of its own: the two pixel planes every partition has, and,
// under a band partition of a multiple of 8 rows (where crt_trace_adaptive works), the adaptive state's second moment Q per
// pixel and its sample count per 8x8 tile -- the tile grid partitioned by crt_layout_rows(ceil(H/8), band/8, world, rank).
enum { PL_RGBA = 0, PL_ACCUM = 1, PL_Q = 2, PL_COUNTS = 3, PL_N = 4 };

// What a CRT_GATHER_PREVIEW records: which of the rank's PREVIEW gathers since the partition it was, and the frame state then.
struct Preview {
    uint64_t count = 0;
    uint32_t adaptive = 0, n = 0;                  // the state; the uniform sample count (0 in the adaptive state)
};

struct LocalGroup {
    int world = 0;
    std::vector<Comm *> member;                    // by rank; null until that rank has joined
    std::vector<uint64_t> posted[PL_N];            // per plane and rank: gathers posted so far
    std::vector<Preview> preview;                  // per rank: its latest PREVIEW gather
};

struct Plane {
    uint32_t elem = 0;                             // bytes per element; 0: this partition has no such plane
    uint32_t W = 0, H = 0, band = 0, rows = 0, rows_max = 0;   // the frame it partitions, this rank's rows of it, the largest rank's
    void *strip = nullptr;                         // this rank's rows, padded to rows_max (pixel planes: bound as the context's output)
    void *full = nullptr;                          // [world][rows_max][W]: the gathered strips
    void *frame = nullptr;                         // [H][W]: assembled frame
    uint64_t n = 0, asm_n = 0;                     // gathers posted by this rank, and assembled
    hipEvent_t ev = nullptr;                       // local transport: after this rank's copies of its latest gather
    hipEvent_t ev_asm = nullptr;                   // ... and after this rank's latest assembly (it reads `full`: a peer's next copy waits for it)
    bool asm_recorded = false;
    size_t strip_bytes() const { return (size_t)std::max(rows_max, 1u) * W * elem; }
};

struct Comm {
    crt_ctx *ctx = nullptr;
    int rank = 0, world = 1, device = 0;
    bool local = false;
    ncclComm_t nccl = nullptr;
    std::shared_ptr<LocalGroup> group;
    char id[CRT_COMM_ID_BYTES] = {0};
    // partition and buffers (valid once crt_comm_partition has run)
    bool partitioned = false;
    uint32_t W = 0, H = 0, band = 0, rows = 0, rows_max = 0;
    Plane pl[PL_N];
    // the latest CRT_GATHER_PREVIEW since the partition (count == 0: none): what the frame-level calls work on
    Preview pv;
    uint32_t pv_epoch = 0;                                   // the context's frame-state epoch at that gather
    uint64_t pv_accum_n = 0;                                 // ... and which gather of the accumulator plane it posted
};
std::map<crt_ctx *, std::unique_ptr<Comm>> g_comms;
std::map<std::string, std::weak_ptr<LocalGroup>> g_groups;
std::atomic<uint64_t> g_local_seq{1};

int fail(crt_ctx *c, int code, const std::string &msg) { return crt_internal_fail(c, code, msg.c_str()); }
#define CHIP(c, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail(c, e_ == hipErrorOutOfMemory ? CRT_ENOMEM : CRT_EDEVICE, std::string(#call ": ") + hipGetErrorString(e_)); } while (0)

Comm *find(crt_ctx *c)
{
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_comms.find(c);
    return it == g_comms.end() ? nullptr : it->second.get();
}

void free_buffers(Comm &m)
{
    for (Plane &q : m.pl) {
        for (void **p : {&q.strip, &q.full, &q.frame})
            if (*p) { (void)hipFree(*p); *p = nullptr; }
        q.elem = 0;
    }
    m.partitioned = false;
}

bool is_local_id(const void *id) { return std::memcmp(id, "CRTLOCAL", 8) == 0; }

// rows of the frame that belong to `part` (the layout crt_set_row_bands / contiguous strips give)
uint32_t rows_of(uint32_t H, uint32_t band, uint32_t parts, uint32_t part)
{
    uint32_t n = 0;
    (void)crt_layout_rows(H, band, parts, part, &n, nullptr);
    return n;
}

// Does the context still render what crt_comm_partition set up?  crt_upload_scene, crt_set_tile and crt_set_row_bands
// unbind the strips (and may change W and H), crt_bind_output with other pointers does so by itself: the partition is
// then STALE.  Asked of the context through the public ABI at every entry, so nothing has to tell the communicator.
// (The strips stay allocated while stale, so no buffer of the context's own can take their addresses.)
bool bound_to_strips(crt_ctx *c, const Comm *m)
{
    void *a = nullptr, *r = nullptr;
    return m->partitioned && crt_device_buffers(c, &a, &r) == CRT_OK && a == m->pl[PL_ACCUM].strip && r == m->pl[PL_RGBA].strip;
}

bool current(crt_ctx *c, const Comm *m)
{
    if (!bound_to_strips(c, m)) return false;
    uint32_t wh[2] = {0, 0}, t[4] = {0, 0, 0, 0};
    if (crt_image_size(c, wh) != CRT_OK || wh[0] != m->W || wh[1] != m->H) return false;
    return crt_tile(c, t) == CRT_OK && t[2] == m->W && t[3] == m->rows;
}

// What crt_gather, crt_read_frame_* and crt_frame_device_buffers answer before they touch anything.
int refuse_unless_current(crt_ctx *c, const Comm *m, const char *who)
{
    if (!m || !m->partitioned) return fail(c, CRT_ESTATE, std::string(who) + ": crt_comm_init and crt_comm_partition first");
    if (!current(c, m))
        return fail(c, CRT_ESTATE, std::string(who) + ": the partition is stale (crt_upload_scene, crt_set_tile, crt_set_row_bands or "
                                   "crt_bind_output since): call crt_comm_partition again");
    return CRT_OK;
}

}  // namespace

extern "C" {

int crt_layout_rows(uint32_t H, uint32_t band_rows, uint32_t parts, uint32_t part, uint32_t *n_rows, uint32_t *global_rows)
{
    if (parts == 0 || part >= parts || !n_rows) return CRT_EINVAL;
    uint32_t n = 0;
    if (band_rows == 0) {                                      // contiguous strips of ceil(H / parts) rows
        const uint32_t per = (H + parts - 1) / parts;
        const uint32_t y0 = std::min<uint64_t>((uint64_t)part * per, H), y1 = std::min<uint64_t>((uint64_t)y0 + per, H);
        for (uint32_t y = y0; y < y1; y++, n++) if (global_rows) global_rows[n] = y;
    } else {                                                   // bands of band_rows rows dealt round-robin
        for (uint64_t b = part; b * band_rows < H; b += parts)
            for (uint32_t y = (uint32_t)(b * band_rows); y < H && y < (b + 1) * band_rows; y++, n++)
                if (global_rows) global_rows[n] = y;
    }
    *n_rows = n;
    return CRT_OK;
}

int crt_comm_unique_id(void *out, int transport)
{
    if (!out) return CRT_EINVAL;
    std::memset(out, 0, CRT_COMM_ID_BYTES);
    if (transport == CRT_COMM_LOCAL) {
        const uint64_t seq = g_local_seq.fetch_add(1);
        std::memcpy(out, "CRTLOCAL", 8);
        std::memcpy((char *)out + 8, &seq, sizeof seq);
        return CRT_OK;
    }
    if (transport != CRT_COMM_RCCL) return crt_internal_fail(nullptr, CRT_EINVAL, "crt_comm_unique_id: unknown transport");
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_rccl.load()) return crt_internal_fail(nullptr, CRT_EDEVICE, ("crt_comm_unique_id: " + g_rccl.err).c_str());
    ncclUniqueId id;
    const ncclResult_t r = g_rccl.GetUniqueId(&id);
    if (r != ncclSuccess) return crt_internal_fail(nullptr, CRT_EDEVICE, (std::string("ncclGetUniqueId: ") + g_rccl.GetErrorString(r)).c_str());
    static_assert(sizeof(ncclUniqueId) == CRT_COMM_ID_BYTES, "id size");
    std::memcpy(out, &id, sizeof id);
    return CRT_OK;
}

int crt_comm_init(crt_ctx *c, const void *id, int rank, int world)
{
    if (!c || !id) return CRT_EINVAL;
    if (world < 1 || rank < 0 || rank >= world || world > 1024) return fail(c, CRT_EINVAL, "crt_comm_init: need 0 <= rank < world <= 1024");
    if (find(c)) return fail(c, CRT_ESTATE, "crt_comm_init: the context already has a communicator (crt_comm_destroy first)");
    int device = 0;
    { int rc = crt_get_device(c, &device); if (rc) return rc; }
    CHIP(c, hipSetDevice(device));
    std::unique_ptr<Comm> m(new Comm());
    m->ctx = c; m->rank = rank; m->world = world; m->device = device;
    std::memcpy(m->id, id, CRT_COMM_ID_BYTES);
    m->local = is_local_id(id);
    // (the events first: nothing below may fail once the rank has joined its group or its RCCL communicator exists)
    auto drop_events = [&]() {
        for (Plane &q : m->pl)
            for (hipEvent_t *e : {&q.ev, &q.ev_asm}) if (*e) { (void)hipEventDestroy(*e); *e = nullptr; }
    };
    for (Plane &q : m->pl)
        if (hipEventCreateWithFlags(&q.ev, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&q.ev_asm, hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            drop_events();
            return fail(c, CRT_EDEVICE, "crt_comm_init: hipEventCreate failed");
        }
    if (m->local) {
        std::lock_guard<std::mutex> lk(g_mu);
        const std::string key((const char *)id, CRT_COMM_ID_BYTES);
        std::shared_ptr<LocalGroup> g = g_groups[key].lock();
        if (!g) {
            g = std::make_shared<LocalGroup>();
            g->world = world; g->member.assign((size_t)world, nullptr);
            for (auto &v : g->posted) v.assign((size_t)world, 0);
            g->preview.assign((size_t)world, Preview());
            g_groups[key] = g;
        }
        if (g->world != world) { drop_events(); return fail(c, CRT_EINVAL, "crt_comm_init: the ranks of one id disagree about the world size"); }
        if (g->member[(size_t)rank]) { drop_events(); return fail(c, CRT_EINVAL, "crt_comm_init: that rank of the id is taken"); }
        g->member[(size_t)rank] = m.get();
        m->group = g;
    } else {
        {
            std::lock_guard<std::mutex> lk(g_mu);
            if (!g_rccl.load()) { drop_events(); return fail(c, CRT_EDEVICE, "crt_comm_init: " + g_rccl.err); }
        }
        ncclUniqueId uid;
        std::memcpy(&uid, id, sizeof uid);
        const ncclResult_t r = g_rccl.CommInitRank(&m->nccl, world, uid, rank);   // (collective: every rank of the id calls it)
        if (r != ncclSuccess) { drop_events(); return fail(c, CRT_EDEVICE, std::string("ncclCommInitRank: ") + g_rccl.GetErrorString(r)); }
    }
    std::lock_guard<std::mutex> lk(g_mu);
    g_comms[c] = std::move(m);
    return CRT_OK;
}

int crt_comm_destroy(crt_ctx *c)
{
    std::unique_ptr<Comm> m;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        auto it = g_comms.find(c);
        if (it == g_comms.end()) return CRT_OK;
        m = std::move(it->second);
        g_comms.erase(it);
        if (m->group) m->group->member[(size_t)m->rank] = nullptr;
    }
    (void)hipSetDevice(m->device);
    void *st = nullptr;
    if (crt_get_stream(c, &st) == CRT_OK) (void)hipStreamSynchronize((hipStream_t)st);
    if (bound_to_strips(c, m.get())) (void)crt_bind_output(c, nullptr, nullptr);   // (a stale partition: the outputs are the application's)
    free_buffers(*m);
    if (m->nccl) (void)g_rccl.CommDestroy(m->nccl);
    for (Plane &q : m->pl)
        for (hipEvent_t e : {q.ev, q.ev_asm}) if (e) (void)hipEventDestroy(e);
    return CRT_OK;
}

// called by crt_destroy
void crt_comm_on_destroy(crt_ctx *c) { (void)crt_comm_destroy(c); }

int crt_comm_partition(crt_ctx *c, uint32_t band_rows)
{
    Comm *m = find(c);
    if (!m) return fail(c, CRT_ESTATE, "crt_comm_partition: crt_comm_init first");
    uint32_t wh[2];
    { int rc = crt_image_size(c, wh); if (rc) return rc; }
    const uint32_t W = wh[0], H = wh[1];
    if (band_rows > 65536u) return fail(c, CRT_EINVAL, "crt_comm_partition: band_rows must be 0 (contiguous strips) .. 65536");
    CHIP(c, hipSetDevice(m->device));
    if (m->partitioned) { int rc = crt_bind_output(c, nullptr, nullptr); if (rc) return rc; }
    free_buffers(*m);
    uint32_t rows_max = 0;
    for (int p = 0; p < m->world; p++) rows_max = std::max(rows_max, rows_of(H, band_rows, (uint32_t)m->world, (uint32_t)p));
    m->W = W; m->H = H; m->band = band_rows; m->rows_max = rows_max;
    m->rows = rows_of(H, band_rows, (uint32_t)m->world, (uint32_t)m->rank);
    int rc;
    if (band_rows) rc = crt_set_row_bands(c, band_rows, (uint32_t)m->world, (uint32_t)m->rank);
    else {
        const uint32_t per = (H + (uint32_t)m->world - 1) / (uint32_t)m->world;
        const uint32_t y0 = std::min<uint64_t>((uint64_t)m->rank * per, H);
        rc = crt_set_tile(c, 0, y0, W, std::min<uint64_t>((uint64_t)y0 + per, H));
    }
    if (rc) return rc;
    // the planes: the two of the pixels, and where crt_trace_adaptive works (every local 8x8 tile one of the frame's) Q and
    // the tile counts, the tile grid being a small frame partitioned the same way with bands of band_rows / 8 tile rows
    const bool tiles_align = band_rows && band_rows % 8u == 0;
    for (int k : {PL_RGBA, PL_ACCUM, PL_Q}) {
        if (k == PL_Q && !tiles_align) continue;
        Plane &q = m->pl[k];
        q.elem = k == PL_ACCUM ? 16u : 4u;
        q.W = W; q.H = H; q.band = band_rows; q.rows = m->rows; q.rows_max = rows_max;
    }
    if (tiles_align) {
        Plane &t = m->pl[PL_COUNTS];
        t.elem = 4u; t.W = (W + 7u) / 8u; t.H = (H + 7u) / 8u; t.band = band_rows / 8u;
        t.rows = rows_of(t.H, t.band, (uint32_t)m->world, (uint32_t)m->rank);
        t.rows_max = 0;
        for (int p = 0; p < m->world; p++) t.rows_max = std::max(t.rows_max, rows_of(t.H, t.band, (uint32_t)m->world, (uint32_t)p));
        if (t.rows != (m->rows + 7u) / 8u) return fail(c, CRT_EDEVICE, "crt_comm_partition: the tile rows of this rank are not its rows' tiles");
    }
    for (Plane &q : m->pl) {
        q.n = q.asm_n = 0; q.asm_recorded = false;
        if (!q.elem) continue;
        const size_t strip = q.strip_bytes(), frame = (size_t)std::max(q.H, 1u) * q.W * q.elem;
        CHIP(c, hipMalloc(&q.strip, strip)); CHIP(c, hipMalloc(&q.full, strip * (size_t)m->world)); CHIP(c, hipMalloc(&q.frame, frame));
        CHIP(c, hipMemset(q.strip, 0, strip)); CHIP(c, hipMemset(q.frame, 0, frame));
    }
    m->partitioned = true;
    m->pv = Preview();
    if (m->group) {
        std::lock_guard<std::mutex> lk(g_mu);
        for (auto &v : m->group->posted) v[(size_t)m->rank] = 0;
        m->group->preview[(size_t)m->rank] = Preview();
    }
    // the context renders straight into the padded strips (and its accumulator starts at zero there)
    return crt_bind_output(c, m->pl[PL_ACCUM].strip, m->pl[PL_RGBA].strip);
}

// Post one gather of this rank's strip on the context's stream: what is in the strip THEN, in stream order -- after a
// crt_sync every sample requested so far, in the middle of a pipelined run the latest complete frame (crt_trace's contract
// for bound outputs).
static int gather_one(crt_ctx *c, Comm *m, int plane)
{
    void *st = nullptr;
    { int rc = crt_get_stream(c, &st); if (rc) return rc; }
    hipStream_t s = (hipStream_t)st;
    Plane &q = m->pl[plane];
    const size_t strip_bytes = q.strip_bytes();
    const void *src = q.strip;
    if (!m->local) {
        const ncclResult_t r = g_rccl.AllGather(src, q.full, strip_bytes, ncclUint8, m->nccl, s);
        if (r != ncclSuccess) return fail(c, CRT_EDEVICE, std::string("ncclAllGather: ") + g_rccl.GetErrorString(r));
        q.n++;
        return CRT_OK;
    }
    // local transport: this rank's strip into slot `rank` of every member's gather buffer
    std::vector<Comm *> peers;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        peers = m->group->member;
    }
    for (Comm *p : peers) {
        if (!p || !p->partitioned) return fail(c, CRT_ESTATE, "crt_gather: every rank of the communicator must have called crt_comm_partition");
        if (p->rows_max != m->rows_max || p->W != m->W || p->H != m->H || p->band != m->band)
            return fail(c, CRT_EINVAL, "crt_gather: the ranks of the communicator disagree about the partition");
        Plane &pq = p->pl[plane];
        if (pq.elem != q.elem || pq.strip_bytes() != strip_bytes)   // (the same partition gives every rank the same planes)
            return fail(c, CRT_EINVAL, "crt_gather: the ranks of the communicator disagree about the partition");
        char *pd = (char *)pq.full + (size_t)m->rank * strip_bytes;
        // (the peer's assembly of the PREVIOUS gather reads the buffer this copy writes: behind it, whatever the streams)
        if (p != m && pq.asm_recorded) CHIP(c, hipStreamWaitEvent(s, pq.ev_asm, 0));
        CHIP(c, hipMemcpyPeerAsync(pd, p->device, src, m->device, strip_bytes, s));
    }
    CHIP(c, hipEventRecord(q.ev, s));
    std::lock_guard<std::mutex> lk(g_mu);
    q.n++;
    m->group->posted[plane][(size_t)m->rank] = q.n;
    return CRT_OK;
}

// CRT_GATHER_PREVIEW: what the frame-level calls need, in one step.  A sync point for this context (what is in flight is
// finished, as crt_read_adaptive finishes it), then on its stream the accumulator's gather -- the plain one, so
// crt_read_frame_accum sees it too -- and in the adaptive state those of Q and of the tile counts, staged from the
// context's own unpadded buffers into the padded strips.  The frame state is recorded beside it.
static int gather_preview(crt_ctx *c, Comm *m, int what)
{
    uint32_t st[3] = {0, 0, 0};
    void *q_dev = nullptr, *counts_dev = nullptr;
    { int rc = crt_internal_frame_state(c, 1, "crt_gather", st, &q_dev, &counts_dev); if (rc) return rc; }
    const bool adaptive = st[0] != 0;
    if (adaptive && (!m->pl[PL_Q].elem || !m->pl[PL_COUNTS].elem || !q_dev || !counts_dev))
        return fail(c, CRT_ESTATE, "crt_gather: the adaptive state needs a band partition of a multiple of 8 rows");
    if (m->local) {                                            // a peer that has posted this round already must hold the same kind of frame
        std::lock_guard<std::mutex> lk(g_mu);
        for (const Preview &p : m->group->preview)
            if (p.count == m->pv.count + 1 && (p.adaptive != st[0] || p.n != st[1]))
                return fail(c, CRT_EINVAL, "crt_gather: the ranks disagree about the frame state (uniform or adaptive, or the sample count)");
    }
    void *sv = nullptr;
    { int rc = crt_get_stream(c, &sv); if (rc) return rc; }
    hipStream_t s = (hipStream_t)sv;
    if (what & CRT_GATHER_RGBA8) { int rc = gather_one(c, m, PL_RGBA); if (rc) return rc; }
    { int rc = gather_one(c, m, PL_ACCUM); if (rc) return rc; }
    if (adaptive) {
        const void *src[2] = {q_dev, counts_dev};
        const int plane[2] = {PL_Q, PL_COUNTS};
        for (int k = 0; k < 2; k++) {
            const Plane &q = m->pl[plane[k]];
            const size_t bytes = (size_t)q.rows * q.W * q.elem;                // (the strip's padding stays zero)
            if (bytes) CHIP(c, hipMemcpyAsync(q.strip, src[k], bytes, hipMemcpyDeviceToDevice, s));
            { int rc = gather_one(c, m, plane[k]); if (rc) return rc; }
        }
    }
    m->pv.count++; m->pv.adaptive = st[0]; m->pv.n = st[1];
    m->pv_epoch = st[2]; m->pv_accum_n = m->pl[PL_ACCUM].n;
    if (m->local) { std::lock_guard<std::mutex> lk(g_mu); m->group->preview[(size_t)m->rank] = m->pv; }
    return CRT_OK;
}

int crt_gather(crt_ctx *c, int what)
{
    Comm *m = find(c);
    { int rc = refuse_unless_current(c, m, "crt_gather"); if (rc) return rc; }
    if (!(what & (CRT_GATHER_RGBA8 | CRT_GATHER_ACCUM | CRT_GATHER_PREVIEW))) return fail(c, CRT_EINVAL, "crt_gather: nothing to gather");
    CHIP(c, hipSetDevice(m->device));
    if (what & CRT_GATHER_PREVIEW) return gather_preview(c, m, what);          // (it gathers the accumulator itself)
    if (what & CRT_GATHER_RGBA8) { int rc = gather_one(c, m, PL_RGBA); if (rc) return rc; }
    if (what & CRT_GATHER_ACCUM) { int rc = gather_one(c, m, PL_ACCUM); if (rc) return rc; }
    return CRT_OK;
}

// Assemble the frame of the latest gather on this rank's stream (full -> frame: the rows back in image order).
static int assemble(crt_ctx *c, Comm *m, int plane, hipStream_t s)
{
    Plane &q = m->pl[plane];
    uint64_t &done = q.asm_n;
    const uint64_t posted = q.n;
    if (posted == 0) return fail(c, CRT_ESTATE, "crt_read_frame: no crt_gather of that buffer yet");
    if (m->local) {
        // every rank's copies of gather number `posted` must be in: their streams are joined through their events
        std::vector<Comm *> peers;
        {
            std::lock_guard<std::mutex> lk(g_mu);
            for (int p = 0; p < m->world; p++)
                if (m->group->posted[plane][(size_t)p] < posted)
                    return fail(c, CRT_ESTATE, "crt_read_frame: rank " + std::to_string(p) + " of the communicator has not posted its crt_gather yet");
            peers = m->group->member;
        }
        for (Comm *p : peers) if (p && p != m) CHIP(c, hipStreamWaitEvent(s, p->pl[plane].ev, 0));
    }
    if (done != posted) {
        const hipError_t e = crt::launch_assemble(q.full, q.frame, q.elem, q.W, q.H, (uint32_t)m->world, std::max(q.rows_max, 1u), q.band, s);
        if (e != hipSuccess) return fail(c, CRT_EDEVICE, std::string("frame assembly: ") + hipGetErrorString(e));
        done = posted;
        if (m->local) {
            CHIP(c, hipEventRecord(q.ev_asm, s));
            q.asm_recorded = true;
        }
    }
    return CRT_OK;
}

static int read_frame(crt_ctx *c, void *out, bool accum)
{
    const int plane = accum ? PL_ACCUM : PL_RGBA;
    Comm *m = find(c);
    { int rc = refuse_unless_current(c, m, "crt_read_frame"); if (rc) return rc; }
    if (!out) return CRT_EINVAL;
    CHIP(c, hipSetDevice(m->device));
    void *st = nullptr;
    { int rc = crt_get_stream(c, &st); if (rc) return rc; }
    hipStream_t s = (hipStream_t)st;
    { int rc = assemble(c, m, plane, s); if (rc) return rc; }
    const size_t bytes = (size_t)m->W * m->H * (accum ? 16 : 4);
    if (bytes) CHIP(c, hipMemcpyAsync(out, m->pl[plane].frame, bytes, hipMemcpyDeviceToHost, s));
    CHIP(c, hipStreamSynchronize(s));
    return CRT_OK;
}

int crt_read_frame_rgba8(crt_ctx *c, uint8_t *out) { return read_frame(c, out, false); }
int crt_read_frame_accum(crt_ctx *c, float *out) { return read_frame(c, out, true); }

int crt_frame_device_buffers(crt_ctx *c, void **accum_dev, void **rgba8_dev)
{
    Comm *m = find(c);
    { int rc = refuse_unless_current(c, m, "crt_frame_device_buffers"); if (rc) return rc; }
    CHIP(c, hipSetDevice(m->device));
    void *st = nullptr;
    { int rc = crt_get_stream(c, &st); if (rc) return rc; }
    if (accum_dev) { if (m->pl[PL_ACCUM].n) { int rc = assemble(c, m, PL_ACCUM, (hipStream_t)st); if (rc) return rc; } *accum_dev = m->pl[PL_ACCUM].frame; }
    if (rgba8_dev) { if (m->pl[PL_RGBA].n) { int rc = assemble(c, m, PL_RGBA, (hipStream_t)st); if (rc) return rc; } *rgba8_dev = m->pl[PL_RGBA].frame; }
    return CRT_OK;
}

// crt_denoise_api.cpp (crt_denoise_frame, crt_denoise_adaptive_frame, crt_read_frame_adaptive): the frame of the latest
// CRT_GATHER_PREVIEW, or why there is none for this call.  Every refusal comes before anything is enqueued; with
// `assemble_now` the planes are then put in order on the context's stream.  planes[3] = the frame's accumulator, Q and tile
// counts (the last two NULL for a uniform frame); dims[3] = W, H and the uniform sample count.
int crt_internal_comm_frame_view(crt_ctx *c, const char *who, int adaptive, int assemble_now, const void *planes[3], uint32_t dims[3])
{
    Comm *m = find(c);
    { int rc = refuse_unless_current(c, m, who); if (rc) return rc; }
    if (m->pv.count == 0) return fail(c, CRT_ESTATE, std::string(who) + ": no crt_gather(CRT_GATHER_PREVIEW) since crt_comm_partition");
    if ((m->pv.adaptive != 0) != (adaptive != 0))
        return fail(c, CRT_ESTATE, std::string(who) + (m->pv.adaptive ? ": the gathered frame is an adaptive one (per-tile sample counts: crt_denoise_adaptive_frame, crt_read_frame_adaptive)"
                                                                      : ": the gathered frame is a uniform one (crt_denoise_frame filters it)"));
    uint32_t st[3] = {0, 0, 0};
    { int rc = crt_internal_frame_state(c, 0, who, st, nullptr, nullptr); if (rc) return rc; }
    if (st[2] != m->pv_epoch)
        return fail(c, CRT_ESTATE, std::string(who) + ": the context's frame was reset or replaced since the PREVIEW gather (a reset, an edit, the camera): gather again");
    if (m->pl[PL_ACCUM].n != m->pv_accum_n)
        return fail(c, CRT_ESTATE, std::string(who) + ": the accumulator was gathered again since the PREVIEW gather, without the planes that go with it: gather again");
    if (m->local) {
        std::lock_guard<std::mutex> lk(g_mu);
        for (int p = 0; p < m->world; p++) {
            const Preview &pp = m->group->preview[(size_t)p];
            if (pp.count < m->pv.count)
                return fail(c, CRT_ESTATE, std::string(who) + ": rank " + std::to_string(p) + " of the communicator has not posted its crt_gather yet");
            if (pp.count == m->pv.count && (pp.adaptive != m->pv.adaptive || pp.n != m->pv.n))
                return fail(c, CRT_EINVAL, std::string(who) + ": the ranks disagree about the frame state (uniform or adaptive, or the sample count)");
        }
    }
    dims[0] = m->W; dims[1] = m->H; dims[2] = m->pv.n;
    planes[0] = m->pl[PL_ACCUM].frame;
    planes[1] = adaptive ? m->pl[PL_Q].frame : nullptr;
    planes[2] = adaptive ? m->pl[PL_COUNTS].frame : nullptr;
    if (!assemble_now) return CRT_OK;
    CHIP(c, hipSetDevice(m->device));
    void *sv = nullptr;
    { int rc = crt_get_stream(c, &sv); if (rc) return rc; }
    { int rc = assemble(c, m, PL_ACCUM, (hipStream_t)sv); if (rc) return rc; }
    if (adaptive) {
        { int rc = assemble(c, m, PL_Q, (hipStream_t)sv); if (rc) return rc; }
        { int rc = assemble(c, m, PL_COUNTS, (hipStream_t)sv); if (rc) return rc; }
    }
    return CRT_OK;
}

int crt_comm_info(crt_ctx *c, int out[4])
{
    if (!out) return CRT_EINVAL;
    Comm *m = find(c);
    if (!m) { out[0] = 0; out[1] = 1; out[2] = -1; out[3] = 0; return CRT_OK; }
    out[0] = m->rank; out[1] = m->world; out[2] = m->local ? CRT_COMM_LOCAL : CRT_COMM_RCCL; out[3] = (int)m->rows;
    return CRT_OK;
}

// (crt_api.cpp, crt_trace_adaptive.  0: no partition, a stale one is none; 2: bands of a multiple of 8 rows, so every local
// 8x8 tile is one of the frame's and the call works; 1: any other partition, which it refuses)
int crt_internal_comm_partitioned(crt_ctx *c)
{
    Comm *m = find(c);
    if (!m || !current(c, m)) return 0;
    return m->band && m->band % 8u == 0 ? 2 : 1;
}

}  // extern "C"
