// crt_matte_api.cpp -- the entry points of the id mattes (crt_matte.hip): crt_render_mattes and the
// per-primitive id table it reads under CRT_MATTE_OBJECT (crt_set_primitive_ids, crt_read_primitive_ids), with the
// table's side of the scene edits.
#include "crt_ctx.h"

using namespace crt;

namespace crt {

// The table lives on the host beside c->prims; every change drops the device copy, which the next crt_render_mattes of
// source OBJECT makes again.  None of these touches the device otherwise: the upload and the edits allocate there exactly
// what they allocated before there was a table.
void matte_ids_identity(crt_ctx *c)
{
    c->prim_ids.resize(c->prims.size());
    for (size_t i = 0; i < c->prim_ids.size(); i++) c->prim_ids[i] = (uint32_t)i;
    c->d_prim_ids.release();
}

void matte_ids_reserve(crt_ctx *c, size_t n_new)
{
    if (c->prim_ids.capacity() < n_new) c->prim_ids.reserve(std::max(n_new, c->prim_ids.capacity() + c->prim_ids.capacity() / 2));
}

// crt_remove_primitives: the survivors close ranks as the records do, and each keeps its id.
void matte_ids_remove(crt_ctx *c, const crt_prim_range *live, size_t m)
{
    std::vector<uint32_t> &t = c->prim_ids;
    const size_t n = t.size();
    size_t w = 0, r = 0;
    for (size_t j = 0; j <= m; j++) {
        const size_t stop = j < m ? live[j].first : n;
        if (w != r) std::copy(t.begin() + r, t.begin() + stop, t.begin() + w);
        w += stop - r;
        if (j < m) r = (size_t)live[j].first + live[j].count;
    }
    t.resize(w);
    c->d_prim_ids.release();
}

// crt_append_primitives: appended primitive nprim + k gets the id nprim + k (matte_ids_reserve has made room).
void matte_ids_append(crt_ctx *c, uint32_t count)
{
    const size_t n = c->prim_ids.size();
    for (uint32_t k = 0; k < count; k++) c->prim_ids.push_back((uint32_t)(n + k));
    c->d_prim_ids.release();
}

// The device copy of the table for a kernel that reads it (crt_render_mattes of source OBJECT, the `id` plane of the ray
// queries): made if a change has dropped it.
int matte_ids_device(crt_ctx *c)
{
    if (c->d_prim_ids.n >= c->prim_ids.size()) return CRT_OK;
    HIPCHK(c, c->d_prim_ids.alloc(c->prim_ids.size()));
    const hipError_t e = hipMemcpy(c->d_prim_ids.p, c->prim_ids.data(), c->prim_ids.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) c->d_prim_ids.release();
    HIPCHK(c, e);
    return CRT_OK;
}

}  // namespace crt

// the range checks the two table calls share
static int ids_range(crt_ctx *c, const char *what, uint32_t first, uint32_t count, const void *p)
{
    if (!p && count) return fail(c, CRT_EINVAL, "%s: the id array is NULL", what);
    if (!c->have_scene) return fail(c, CRT_ESTATE, "%s: upload a scene first", what);
    if ((uint64_t)first + count > c->prim_ids.size())
        return fail(c, CRT_EINVAL, "%s: range [%u, %llu) outside the scene's %zu primitives", what, first,
                    (unsigned long long)first + count, c->prim_ids.size());
    return CRT_OK;
}

extern "C" {

int crt_set_primitive_ids(crt_ctx *c, uint32_t first, uint32_t count, const uint32_t *ids)
{
    const char *what = "crt_set_primitive_ids";
    if (!c) return CRT_EINVAL;
    CRT_TRY(ids_range(c, what, first, count, ids));
    for (uint32_t k = 0; k < count; k++)
        if (ids[k] == 0xFFFFFFFFu) return fail(c, CRT_EINVAL, "%s: id %u is 0xFFFFFFFF, which means \"no entry\" in the planes", what, k);
    if (!count) return CRT_OK;
    // a call in flight reads the scene, never the table: only crt_render_mattes does, and it has finished (a sync point)
    std::copy(ids, ids + count, c->prim_ids.begin() + first);
    c->d_prim_ids.release();
    return CRT_OK;
}

int crt_read_primitive_ids(crt_ctx *c, uint32_t first, uint32_t count, uint32_t *out)
{
    if (!c) return CRT_EINVAL;
    CRT_TRY(ids_range(c, "crt_read_primitive_ids", first, count, out));
    if (count) std::memcpy(out, c->prim_ids.data() + first, (size_t)count * sizeof(uint32_t));
    return CRT_OK;
}

int crt_render_mattes(crt_ctx *c, uint32_t n_samples, int source, uint32_t slots, const crt_matte_planes *out)
{
    const char *what = "crt_render_mattes";
    if (!c) return CRT_EINVAL;
    if (!out) return fail(c, CRT_EINVAL, "%s: out is NULL", what);
    if (slots < 1 || slots > CRT_MATTE_MAX_SLOTS) return fail(c, CRT_EINVAL, "%s: slots is %u, must be 1..%d", what, slots, CRT_MATTE_MAX_SLOTS);
    if (source != CRT_MATTE_PRIMITIVE && source != CRT_MATTE_OBJECT && source != CRT_MATTE_MATERIAL)
        return fail(c, CRT_EINVAL, "%s: unknown source %d", what, source);
    // crt_render_aovs' refusals, in its order
    CRT_TRY(dn_check_state(c, what, true));
    const bool per_tile = n_samples == 0 && c->as_on;
    if (per_tile && c->as_broken) return as_refuse_broken(c, what);
    if (n_samples == 0 && !c->as_on && c->sample == 0)
        return fail(c, CRT_ESTATE, "%s: n_samples = 0 means the samples the accumulator holds, and it holds none", what);
    const unsigned long long n_max = n_samples ? n_samples : per_tile ? c->as_requested : c->sample;
    if ((unsigned long long)c->sample_offset + n_max > 0xFFFFFFFFull)
        return fail(c, CRT_EINVAL, "%s: sample offset %u + %llu samples pass 2^32 - 1", what, c->sample_offset, n_max);
    CRT_TRY(quiesce(c, false));
    const size_t n = (size_t)c->tw * c->th;
    if (n) {
        // every allocation before the first launch: a failed one leaves nothing enqueued
        crt_ctx::Matte &m = c->matte;
        if (out->ids) CRT_ENSURE(c, m.ids, n * slots);
        if (out->counts) CRT_ENSURE(c, m.counts, n * slots);
        if (out->hits) CRT_ENSURE(c, m.hits, n);
        if (out->overflow) CRT_ENSURE(c, m.overflow, n);
        if (source == CRT_MATTE_OBJECT) CRT_TRY(matte_ids_device(c));
        MatteParams P{};
        P.table = source == CRT_MATTE_OBJECT ? c->d_prim_ids.p : nullptr;
        P.counts = per_tile ? c->as_counts.p : nullptr;
        P.ids = out->ids ? m.ids.p : nullptr;
        P.counts_out = out->counts ? m.counts.p : nullptr;
        P.hits = out->hits ? m.hits.p : nullptr;
        P.overflow = out->overflow ? m.overflow.p : nullptr;
        P.x0 = c->x0; P.y0 = c->y0; P.tw = c->tw; P.th = c->th; P.tiles_x = (c->tw + 7) / 8;
        P.first = c->sample_offset;
        P.n = n_samples ? n_samples : c->sample;
        P.slots = slots;
        P.source = source;
        P.brute = c->accel_mode == CRT_ACCEL_NONE;
        HIPCHK(c, matte_launch(c->sc, P, c->stream));
        if (out->ids) HIPCHK(c, hipMemcpyAsync(out->ids, m.ids.p, n * slots * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        if (out->counts) HIPCHK(c, hipMemcpyAsync(out->counts, m.counts.p, n * slots * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        if (out->hits) HIPCHK(c, hipMemcpyAsync(out->hits, m.hits.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        if (out->overflow) HIPCHK(c, hipMemcpyAsync(out->overflow, m.overflow.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    }
    return dn_finish(c, n, nullptr, nullptr, nullptr);
}

}  // extern "C"
