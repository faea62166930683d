// bio_ranges_host.cpp -- host-side operator mirror over the Arrow C Data Interface
// (see include/bio_ranges_host.h).  Plain C++17; the only dependency is libivx_hip.so.
#include "../../include/bio_ranges_host.h"
#include "../../include/ivx.h"
#include "../../include/ivx_select.h"
#include "../../include/ivx_where.h"
#include "../../include/ivx_nearest.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

struct brh_session {
    ivx_ctx *ctx = nullptr;
    std::string err;
    // NULL contigs: 0 = as the reference treats them (see get_contig), 1 = refuse the batch (opt-in; BIO_STRICT_NULL_CONTIGS=1
    // makes it the default of new sessions)
    int string_cigars = 0;              // brh_session_set_string_cigars: depth() accepts a Utf8 / LargeUtf8 cigar column
    int strict_null_contigs = [] { const char *e = std::getenv("BIO_STRICT_NULL_CONTIGS"); return e && *e && *e != '0' ? 1 : 0; }();
};

namespace {

int fail(brh_session *s, const std::string &m) { if (s) s->err = m; return 1; }

int fail_ivx(brh_session *s, ivx_status st)
{
    return fail(s, std::string(ivx_last_error(s->ctx)) + " (ivx status " + std::to_string(st) + ")");
}

std::string column_list(const ArrowSchema *sch)
{
    std::string o = "[";
    for (int64_t i = 0; i < sch->n_children; i++) {
        if (i) o += ", ";
        o += "\"" + std::string(sch->children[i]->name ? sch->children[i]->name : "") + "\"";
    }
    return o + "]";
}

int find_col(const ArrowSchema *sch, const char *name)
{
    for (int64_t i = 0; i < sch->n_children; i++)
        if (sch->children[i]->name && !std::strcmp(sch->children[i]->name, name)) return (int)i;
    return -1;
}

int64_t null_count(const ArrowArray *a)
{
    if (a->null_count >= 0) return a->null_count;
    if (a->n_buffers < 1 || !a->buffers[0]) return 0;
    const uint8_t *v = (const uint8_t *)a->buffers[0];
    int64_t n = 0;
    for (int64_t i = 0; i < a->length; i++) { int64_t j = i + a->offset; n += !((v[j >> 3] >> (j & 7)) & 1); }
    return n;
}

// ---- ContigArray (array_utils.rs:10-24): Utf8 / LargeUtf8 / Utf8View
struct StrCol {
    int kind = 0;               // 0 Utf8, 1 LargeUtf8, 2 Utf8View
    const ArrowArray *a = nullptr;
    bool has_nulls = false;
    bool null_at(int64_t i) const
    {
        if (!has_nulls) return false;
        const uint8_t *v = (const uint8_t *)a->buffers[0];
        const int64_t j = i + a->offset;
        return !((v[j >> 3] >> (j & 7)) & 1);
    }
    std::string_view at(int64_t i) const
    {
        const int64_t j = i + a->offset;
        if (kind == 0) { const int32_t *o = (const int32_t *)a->buffers[1]; return {(const char *)a->buffers[2] + o[j], (size_t)(o[j + 1] - o[j])}; }
        if (kind == 1) { const int64_t *o = (const int64_t *)a->buffers[1]; return {(const char *)a->buffers[2] + o[j], (size_t)(o[j + 1] - o[j])}; }
        const uint8_t *v = (const uint8_t *)a->buffers[1] + 16 * j;
        int32_t len; std::memcpy(&len, v, 4);
        if (len <= 12) return {(const char *)v + 4, (size_t)len};
        int32_t bi, off; std::memcpy(&bi, v + 8, 4); std::memcpy(&off, v + 12, 4);
        return {(const char *)a->buffers[2 + bi] + off, (size_t)len};
    }
};

int get_contig(brh_session *s, brh_batch t, const char *name, StrCol *out)
{
    const int c = find_col(t.schema, name);
    if (c < 0) return fail(s, "contig column '" + std::string(name) + "' not found in batch with columns: " + column_list(t.schema));
    const char *f = t.schema->children[c]->format;
    out->a = t.array->children[c];
    if (!std::strcmp(f, "u")) out->kind = 0;
    else if (!std::strcmp(f, "U")) out->kind = 1;
    else if (!std::strcmp(f, "vu")) out->kind = 2;
    else return fail(s, "unsupported data type " + std::string(f) + " for contig column '" + name + "'; expected Utf8, LargeUtf8, or Utf8View");
    // NULL contigs.  The reference never looks at the validity bitmap of a contig column: the table functions read
    // `value(i)` (whatever bytes the slot's offsets span: "" for arrays made by the Arrow builders), and the join hashes the
    // key columns with create_hashes, where a NULL is a key of its own that equals only other NULLs (the reference compares
    // hashes, never values: interval_join.rs:857, :922-928).  That is what happens here by default (the callers of
    // build_keys say which of the two); none of the reference's tests pins either, so a session can refuse such batches
    // instead (brh_session_set_strict_null_contigs / BIO_STRICT_NULL_CONTIGS=1).
    out->has_nulls = null_count(out->a) > 0 && out->a->n_buffers >= 1 && out->a->buffers[0];
    if (out->has_nulls && s && s->strict_null_contigs) {
        int64_t row = 0;
        for (int64_t i = 0; i < out->a->length; i++) if (out->null_at(i)) { row = i; break; }
        return fail(s, "contig column '" + std::string(name) + "' contains a NULL at row " + std::to_string(row) + "; NULL contigs are not supported");
    }
    return 0;
}

// ---- PosArray (array_utils.rs:26-172)
struct PosCol { char fmt = 0; const ArrowArray *a = nullptr; };

int get_pos(brh_session *s, brh_batch t, const char *name, const char *label, PosCol *out)
{
    const int c = find_col(t.schema, name);
    if (c < 0) return fail(s, std::string(label) + " column '" + name + "' not found in batch with columns: " + column_list(t.schema));
    const char *f = t.schema->children[c]->format;
    if (std::strlen(f) != 1 || !std::strchr("ilIL", f[0]))
        return fail(s, "unsupported data type " + std::string(f) + " for " + label + " column '" + name + "'; expected Int32, Int64, UInt32, or UInt64");
    out->fmt = f[0]; out->a = t.array->children[c];
    return 0;
}

// PosArray::resolve (array_utils.rs:66-135)
int resolve_i32(brh_session *s, const PosCol &p, std::vector<int32_t> *out)
{
    if (null_count(p.a) > 0) return fail(s, "coordinate column contains null values; nearest requires non-null coordinates");
    const int64_t n = p.a->length, o = p.a->offset;
    out->resize((size_t)n);
    char buf[160];
    for (int64_t i = 0; i < n; i++) {
        if (p.fmt == 'i') { (*out)[i] = ((const int32_t *)p.a->buffers[1])[o + i]; continue; }
        bool ok; long long sv = 0; unsigned long long uv = 0;
        if (p.fmt == 'l') { sv = ((const int64_t *)p.a->buffers[1])[o + i]; ok = sv >= INT32_MIN && sv <= INT32_MAX; }
        else if (p.fmt == 'I') { uv = ((const uint32_t *)p.a->buffers[1])[o + i]; ok = uv <= (unsigned long long)INT32_MAX; sv = (long long)uv; }
        else { uv = ((const uint64_t *)p.a->buffers[1])[o + i]; ok = uv <= (unsigned long long)INT32_MAX; sv = (long long)uv; }
        if (!ok) {
            if (p.fmt == 'l') std::snprintf(buf, sizeof buf, "coordinate value %lld at row %lld overflows i32 (max 2147483647)", sv, (long long)i);
            else std::snprintf(buf, sizeof buf, "coordinate value %llu at row %lld overflows i32 (max 2147483647)", uv, (long long)i);
            return fail(s, buf);
        }
        (*out)[i] = (int32_t)sv;
    }
    return 0;
}

// PosArray::resolve_i64 (array_utils.rs:137-172)
int resolve_i64(brh_session *s, const PosCol &p, std::vector<int64_t> *out)
{
    if (null_count(p.a) > 0) return fail(s, "coordinate column contains null values; requires non-null coordinates");
    const int64_t n = p.a->length, o = p.a->offset;
    out->resize((size_t)n);
    char buf[160];
    for (int64_t i = 0; i < n; i++) {
        switch (p.fmt) {
        case 'i': (*out)[i] = ((const int32_t *)p.a->buffers[1])[o + i]; break;
        case 'l': (*out)[i] = ((const int64_t *)p.a->buffers[1])[o + i]; break;
        case 'I': (*out)[i] = ((const uint32_t *)p.a->buffers[1])[o + i]; break;
        default: {
            const uint64_t v = ((const uint64_t *)p.a->buffers[1])[o + i];
            if (v > (uint64_t)INT64_MAX) {
                std::snprintf(buf, sizeof buf, "coordinate value %llu at row %lld overflows i64 (max 9223372036854775807)", (unsigned long long)v, (long long)i);
                return fail(s, buf);
            }
            (*out)[i] = (int64_t)v;
        }
        }
    }
    return 0;
}

// ---- key dictionary: ids in byte order of the (composite) key strings
struct KeyDict {
    std::vector<std::string> names;                 // id -> name
    std::vector<std::vector<uint32_t>> ids;         // per table: row -> id
};

// what a NULL slot of a key column contributes to the key in the JOIN (a key of its own): a byte string no contig name holds
const std::string_view NULL_KEY("\x1e\x00NULL", 6);

int build_keys(brh_session *s, const std::vector<std::pair<brh_batch, brh_columns>> &tables, KeyDict *kd, bool null_as_key = false)
{
    std::vector<std::vector<std::string>> composite(tables.size());
    std::vector<std::vector<StrCol>> cols(tables.size());
    for (size_t t = 0; t < tables.size(); t++) {
        const brh_columns &c = tables[t].second;
        if (c.n_keys < 1) return fail(s, "at least one key column is required");
        cols[t].resize(c.n_keys);
        for (int k = 0; k < c.n_keys; k++)
            if (get_contig(s, tables[t].first, c.keys[k], &cols[t][k])) return 1;
    }
    std::unordered_map<std::string_view, uint32_t> seen;
    std::vector<std::string_view> uniq;
    auto part = [&](size_t t, size_t k, int64_t i) -> std::string_view {
        return null_as_key && cols[t][k].null_at(i) ? NULL_KEY : cols[t][k].at(i);
    };
    auto key_of = [&](size_t t, int64_t i, std::string &scratch) -> std::string_view {
        if (cols[t].size() == 1) return part(t, 0, i);
        scratch.clear();
        for (size_t k = 0; k < cols[t].size(); k++) { if (k) scratch.push_back('\x1f'); scratch.append(part(t, k, i)); }
        return scratch;
    };
    // pass 1: unique keys (composite keys are materialised once per table).  Rows of one contig come in runs in
    // coordinate-sorted tables: a key equal to the previous row's is not looked up again.
    for (size_t t = 0; t < tables.size(); t++) {
        const int64_t n = tables[t].first.array->length;
        if (cols[t].size() > 1) {
            composite[t].resize((size_t)n);
            std::string scratch;
            for (int64_t i = 0; i < n; i++) composite[t][i] = std::string(key_of(t, i, scratch));
        }
        std::string_view last; bool have = false;
        for (int64_t i = 0; i < n; i++) {
            std::string_view k = cols[t].size() > 1 ? std::string_view(composite[t][i]) : part(t, 0, i);
            if (have && k == last) continue;
            last = k; have = true;
            if (seen.emplace(k, 0).second) uniq.push_back(k);
        }
    }
    std::sort(uniq.begin(), uniq.end());             // byte-lexicographic, as String::cmp (grouped_stream.rs:111)
    for (uint32_t i = 0; i < uniq.size(); i++) seen[uniq[i]] = i;
    kd->names.assign(uniq.begin(), uniq.end());
    kd->ids.resize(tables.size());
    // pass 2: ids.  Names of up to 7 bytes ("chr1" ... ) are compared and looked up as one packed 64-bit word.
    auto pack = [](std::string_view k) -> uint64_t { uint64_t w = 0; std::memcpy(&w, k.data(), k.size()); return w | ((uint64_t)(k.size() + 1) << 56); };
    std::unordered_map<uint64_t, uint32_t> short_ids;
    for (const auto &kv : seen) if (kv.first.size() <= 7) short_ids.emplace(pack(kv.first), kv.second);
    for (size_t t = 0; t < tables.size(); t++) {
        const int64_t n = tables[t].first.array->length;
        kd->ids[t].resize((size_t)n);
        std::string_view last; uint64_t last_packed = 0; uint32_t last_id = 0; bool have = false;
        for (int64_t i = 0; i < n; i++) {
            std::string_view k = cols[t].size() > 1 ? std::string_view(composite[t][i]) : part(t, 0, i);
            if (k.size() <= 7) {
                const uint64_t w = pack(k);
                if (w != last_packed) { last_id = short_ids.find(w)->second; last_packed = w; have = false; }
            } else if (!have || k != last) {
                last_id = seen[k]; last = k; have = true; last_packed = 0;
            }
            kd->ids[t][i] = last_id;
        }
    }
    return 0;
}

// ---- Arrow output helpers
struct OutPriv {
    std::vector<void *> bufs; const void *ptrs[4] = {nullptr, nullptr, nullptr, nullptr}; char *fmt = nullptr; ArrowArray *dict = nullptr;
    std::vector<ArrowArray *> children;                 // nested outputs (struct / list): owned, released with the parent
};

void release_array(ArrowArray *a)
{
    if (!a || !a->release) return;
    OutPriv *p = (OutPriv *)a->private_data;
    for (void *b : p->bufs) std::free(b);
    if (p->dict) { if (p->dict->release) p->dict->release(p->dict); std::free(p->dict); }
    for (ArrowArray *c : p->children) { if (c->release) c->release(c); std::free(c); }
    delete p;
    a->release = nullptr;
}
void release_schema(ArrowSchema *sc)
{
    if (!sc || !sc->release) return;
    std::free((void *)sc->format); std::free((void *)sc->name);
    if (sc->dictionary) { if (sc->dictionary->release) sc->dictionary->release(sc->dictionary); std::free(sc->dictionary); }
    for (int64_t c = 0; c < sc->n_children; c++) { if (sc->children[c]->release) sc->children[c]->release(sc->children[c]); std::free(sc->children[c]); }
    std::free(sc->children);
    sc->release = nullptr;
}

void make_schema(ArrowSchema *sc, const char *fmt, const char *name, bool nullable)
{
    std::memset(sc, 0, sizeof *sc);
    sc->format = strdup(fmt); sc->name = strdup(name); sc->flags = nullable ? 2 : 0;   // ARROW_FLAG_NULLABLE
    sc->release = release_schema;
}

// fixed-width column; validity (may be null) is one byte per row, converted to a bitmap
template <typename T>
void make_primitive(ArrowArray *a, const T *data, int64_t n, const uint8_t *valid)
{
    std::memset(a, 0, sizeof *a);
    OutPriv *p = new OutPriv();
    T *d = (T *)std::malloc((size_t)(n ? n : 1) * sizeof(T));
    if (n) std::memcpy(d, data, (size_t)n * sizeof(T));
    p->bufs.push_back(d);
    uint8_t *bm = nullptr; int64_t nulls = 0;
    if (valid) {
        bm = (uint8_t *)std::calloc((size_t)(n + 7) / 8 + 1, 1);
        for (int64_t i = 0; i < n; i++) { if (valid[i]) bm[i >> 3] |= (uint8_t)(1u << (i & 7)); else nulls++; }
        p->bufs.push_back(bm);
    }
    p->ptrs[0] = nulls ? bm : nullptr; p->ptrs[1] = d;
    a->length = n; a->null_count = nulls; a->n_buffers = 2; a->buffers = p->ptrs; a->private_data = p; a->release = release_array;
}

void make_utf8(ArrowArray *a, const std::vector<std::string> &names, const uint32_t *ids, int64_t n)
{
    std::memset(a, 0, sizeof *a);
    OutPriv *p = new OutPriv();
    int32_t *off = (int32_t *)std::malloc((size_t)(n + 1) * sizeof(int32_t));
    size_t total = 0;
    for (int64_t i = 0; i < n; i++) { off[i] = (int32_t)total; total += names[ids[i]].size(); }
    off[n] = (int32_t)total;
    char *data = (char *)std::malloc(total ? total : 1);
    for (int64_t i = 0; i < n; i++) std::memcpy(data + off[i], names[ids[i]].data(), names[ids[i]].size());
    p->bufs.push_back(off); p->bufs.push_back(data);
    p->ptrs[0] = nullptr; p->ptrs[1] = off; p->ptrs[2] = data;
    a->length = n; a->n_buffers = 3; a->buffers = p->ptrs; a->private_data = p; a->release = release_array;
}

struct Side32 { std::vector<int32_t> s, e; };
int load_side32(brh_session *s, brh_batch t, const brh_columns &c, Side32 *o)
{
    PosCol ps, pe;
    if (get_pos(s, t, c.start, "start", &ps) || get_pos(s, t, c.end, "end", &pe)) return 1;
    return resolve_i32(s, ps, &o->s) || resolve_i32(s, pe, &o->e);
}
struct Side64 { std::vector<int64_t> s, e; };
int load_side64(brh_session *s, brh_batch t, const brh_columns &c, Side64 *o)
{
    PosCol ps, pe;
    if (get_pos(s, t, c.start, "start", &ps) || get_pos(s, t, c.end, "end", &pe)) return 1;
    return resolve_i64(s, ps, &o->s) || resolve_i64(s, pe, &o->e);
}

struct IndexGuard { ivx_index *ix = nullptr; ~IndexGuard() { if (ix) ivx_index_free(ix); } };

// the join types that read the build side's match marks (bio_ranges_host.h)
bool join_marks_build(int jt) { return jt >= BRH_JOIN_LEFT_SEMI && jt <= BRH_JOIN_FULL; }
bool join_null_build(int jt) { return jt == BRH_JOIN_RIGHT || jt == BRH_JOIN_FULL; }    // unmatched probe rows, build_idx NULL
bool join_null_probe(int jt) { return jt == BRH_JOIN_LEFT || jt == BRH_JOIN_FULL; }     // unmatched build rows, probe_idx NULL

// the build rows whose bit in `marks` (nb bits, host words) is set / clear, ascending: ONE ivx_bits_select
int select_build_rows(brh_session *s, const std::vector<uint32_t> &marks, uint64_t nb, bool want_set, std::vector<uint32_t> *rows)
{
    rows->assign(nb ? nb : 1, 0u);
    uint64_t m = 0;
    const ivx_status st = ivx_bits_select(s->ctx, IVX_MEM_HOST, marks.data(), nb, want_set ? 1 : 0, rows->data(), nb, &m);
    if (st != IVX_OK) return fail_ivx(s, st);
    rows->resize(m);
    return 0;
}

// an overlap threshold of the table layer as the entries of ivx_where.h take it (null stays null: the plain call)
struct WhereArg {
    ivx_overlap_where w{};
    const ivx_overlap_where *p = nullptr;
    explicit WhereArg(const brh_overlap_where *b)
    {
        if (!b) return;
        w.min_bases = b->min_bases; w.probe_num = b->probe_num; w.probe_den = b->probe_den;
        w.build_num = b->build_num; w.build_den = b->build_den; w.either = b->either;
        p = &w;
    }
    bool asks() const { return p && (w.min_bases > 0 || w.probe_num || w.build_num); }
};

// probe rows with a match: ivx_probe_exists, or under a threshold the exists bytes of ivx_probe_overlap_count_where
ivx_status probe_exists(brh_session *s, const ivx_index *ix, const uint32_t *pk, const int32_t *ps, const int32_t *pe, uint64_t np,
                        const ivx_overlap_where *w, uint8_t *ex)
{
    if (!w) return ivx_probe_exists(s->ctx, ix, IVX_MEM_HOST, pk, ps, pe, np, ex);
    return ivx_probe_overlap_count_where(s->ctx, ix, IVX_MEM_HOST, pk, ps, pe, np, w, nullptr, ex, nullptr);
}

// the Inner pairs of one batch (count, then fill; under a threshold then ivx_pairs_where over the build side's columns bs / be),
// and behind them the probe rows without a match, build_idx NULL (Right / Full)
int join_pairs(brh_session *s, const ivx_index *ix, const uint32_t *pk, const int32_t *ps, const int32_t *pe, uint64_t np, bool null_build,
               std::vector<uint32_t> *bi, std::vector<uint32_t> *pi, std::vector<uint8_t> *bvalid, uint64_t *n_pairs,
               const ivx_overlap_where *w = nullptr, const int32_t *bs = nullptr, const int32_t *be = nullptr, uint64_t nb = 0)
{
    uint64_t total = 0, written = 0;
    ivx_status st = ivx_probe_overlap_count(s->ctx, ix, IVX_MEM_HOST, pk, ps, pe, np, nullptr, &total);
    if (st != IVX_OK) return fail_ivx(s, st);
    bi->assign(total ? total : 1, 0u); pi->assign(total ? total : 1, 0u);
    st = ivx_probe_overlap_fill(s->ctx, ix, IVX_MEM_HOST, pk, ps, pe, np, bi->data(), pi->data(), total, &written);
    if (st != IVX_OK) return fail_ivx(s, st);
    if (w) {
        std::vector<uint32_t> fb(written ? written : 1), fp(written ? written : 1);
        uint64_t kept = 0;
        st = ivx_pairs_where(s->ctx, IVX_MEM_HOST, bi->data(), pi->data(), written, bs, be, nb, ps, pe, np, w,
                             written ? fb.data() : nullptr, written ? fp.data() : nullptr, written, &kept);
        if (st != IVX_OK) return fail_ivx(s, st);
        bi->swap(fb); pi->swap(fp);
        written = kept;
    }
    bi->resize(written); pi->resize(written);
    *n_pairs = written;
    if (null_build) {
        std::vector<uint8_t> ex(np ? np : 1);
        st = probe_exists(s, ix, pk, ps, pe, np, w, ex.data());
        if (st != IVX_OK) return fail_ivx(s, st);
        bvalid->assign(written, 1);
        for (uint64_t i = 0; i < np; i++) if (!ex[i]) { bi->push_back(0u); pi->push_back((uint32_t)i); bvalid->push_back(0); }
    }
    return 0;
}

}  // namespace

extern "C" int brh_session_create(int device_ordinal, brh_session **out)
{
    if (!out) return 1;
    brh_session *s = new brh_session();
    ivx_status st = ivx_ctx_create(device_ordinal, &s->ctx);
    if (st != IVX_OK) { delete s; *out = nullptr; return (int)st; }   // no CPU fallback
    *out = s;
    return 0;
}
extern "C" void brh_session_free(brh_session *s) { if (s) { ivx_ctx_free(s->ctx); delete s; } }
extern "C" const char *brh_last_error(const brh_session *s) { return s ? s->err.c_str() : "null session"; }

extern "C" int brh_check_position_column(brh_session *s, brh_batch table, const char *column, int as_i64, char *errbuf, int errbuf_len)
{
    brh_session tmp;
    brh_session *u = s ? s : &tmp;
    PosCol p;
    int rc = get_pos(u, table, column, "start", &p);
    if (!rc) {
        if (as_i64) { std::vector<int64_t> v; rc = resolve_i64(u, p, &v); }
        else { std::vector<int32_t> v; rc = resolve_i32(u, p, &v); }
    }
    if (rc && errbuf && errbuf_len > 0) std::snprintf(errbuf, (size_t)errbuf_len, "%s", u->err.c_str());
    return rc;
}

extern "C" int brh_check_contig_column(brh_session *s, brh_batch table, const char *column, char *errbuf, int errbuf_len)
{
    brh_session tmp;
    brh_session *u = s ? s : &tmp;
    StrCol c;
    const int rc = get_contig(u, table, column, &c);
    if (rc && errbuf && errbuf_len > 0) std::snprintf(errbuf, (size_t)errbuf_len, "%s", u->err.c_str());
    return rc;
}

extern "C" int brh_session_metrics(brh_session *s, ivx_metrics *out)
{
    if (!s || !out) return 1;
    return ivx_ctx_metrics(s->ctx, out) == IVX_OK ? 0 : 1;
}

extern "C" int brh_session_set_strict_null_contigs(brh_session *s, int on)
{
    if (!s) return 1;
    s->strict_null_contigs = on != 0;
    return 0;
}

extern "C" int brh_session_set_string_cigars(brh_session *s, int on)
{
    if (!s) return 1;
    s->string_cigars = on != 0;
    return 0;
}

extern "C" int brh_session_reserved_bytes(brh_session *s, uint64_t *out)
{
    if (!s || !out) return 1;
    *out = ivx_ctx_reserved_bytes(s->ctx);
    return 0;
}

extern "C" int brh_session_set_memory_limit(brh_session *s, uint64_t bytes)
{
    if (!s) return 1;
    return ivx_ctx_set_memory_limit(s->ctx, bytes) == IVX_OK ? 0 : 1;
}

extern "C" int brh_count_overlaps(brh_session *s, brh_batch left, brh_columns lcols, brh_batch right, brh_columns rcols,
                                  int filter_op, int coverage, ArrowArray *out, ArrowSchema *out_schema)
{
    if (!s) return 1;
    KeyDict kd; Side32 L, R;
    if (build_keys(s, {{left, lcols}, {right, rcols}}, &kd) || load_side32(s, left, lcols, &L) || load_side32(s, right, rcols, &R)) return 1;
    const uint32_t nk = (uint32_t)std::max<size_t>(kd.names.size(), 1);
    IndexGuard g;
    ivx_status st = ivx_index_build(s->ctx, coverage ? IVX_KIND_COVERAGE : IVX_KIND_COUNT, IVX_MEM_HOST, kd.ids[0].data(),
                                    L.s.data(), L.e.data(), L.s.size(), nk, &g.ix);
    if (st != IVX_OK) return fail_ivx(s, st);
    std::vector<int64_t> col(R.s.size());
    st = (coverage ? ivx_probe_coverage : ivx_probe_count)(s->ctx, g.ix, IVX_MEM_HOST, kd.ids[1].data(), R.s.data(), R.e.data(),
                                                           R.s.size(), filter_op == BRH_STRICT, col.data());
    if (st != IVX_OK) return fail_ivx(s, st);
    make_primitive<int64_t>(out, col.data(), (int64_t)col.size(), nullptr);
    make_schema(out_schema, "l", coverage ? "coverage" : "count", false);      // count_overlaps.rs:60-66
    return 0;
}

// brh_nearest is brh_nearest_dir on either side and without a cap (ivx_probe_nearest_dir is ivx_probe_nearest then)
extern "C" int brh_nearest(brh_session *s, brh_batch left, brh_columns lcols, brh_batch right, brh_columns rcols,
                           int filter_op, uint32_t k, int include_overlaps, int compute_distance,
                           ArrowArray *left_idx, ArrowSchema *left_idx_schema, ArrowArray *right_idx, ArrowSchema *right_idx_schema,
                           ArrowArray *distance, ArrowSchema *distance_schema)
{
    return brh_nearest_dir(s, left, lcols, right, rcols, filter_op, k, include_overlaps, compute_distance, BRH_NEAR_ANY, -1,
                           left_idx, left_idx_schema, right_idx, right_idx_schema, distance, distance_schema);
}

extern "C" int brh_nearest_dir(brh_session *s, brh_batch left, brh_columns lcols, brh_batch right, brh_columns rcols,
                               int filter_op, uint32_t k, int include_overlaps, int compute_distance, int direction, int64_t max_distance,
                               ArrowArray *left_idx, ArrowSchema *left_idx_schema, ArrowArray *right_idx, ArrowSchema *right_idx_schema,
                               ArrowArray *distance, ArrowSchema *distance_schema)
{
    if (!s) return 1;
    KeyDict kd; Side32 L, R;
    if (build_keys(s, {{left, lcols}, {right, rcols}}, &kd) || load_side32(s, left, lcols, &L) || load_side32(s, right, rcols, &R)) return 1;
    const uint32_t nk = (uint32_t)std::max<size_t>(kd.names.size(), 1);
    IndexGuard g;
    ivx_status st = ivx_index_build(s->ctx, IVX_KIND_NEAREST, IVX_MEM_HOST, kd.ids[0].data(), L.s.data(), L.e.data(), L.s.size(), nk, &g.ix);
    if (st != IVX_OK) return fail_ivx(s, st);
    const uint64_t cap = R.s.size() * (uint64_t)std::max<uint32_t>(k, 1);
    std::vector<uint32_t> bi(cap ? cap : 1), pi(cap ? cap : 1);
    std::vector<int64_t> di(compute_distance ? (cap ? cap : 1) : 0);
    uint64_t rows = 0;
    st = ivx_probe_nearest_dir(s->ctx, g.ix, IVX_MEM_HOST, kd.ids[1].data(), R.s.data(), R.e.data(), R.s.size(), filter_op == BRH_STRICT, k,
                               include_overlaps, direction, max_distance, bi.data(), pi.data(), compute_distance ? di.data() : nullptr, cap, &rows);
    if (st != IVX_OK) return fail_ivx(s, st);
    std::vector<uint8_t> valid(rows ? rows : 1);
    for (uint64_t i = 0; i < rows; i++) { valid[i] = bi[i] != IVX_NULL_IDX; if (!valid[i]) bi[i] = 0; }   // nearest.rs:378-379
    make_primitive<uint32_t>(left_idx, bi.data(), (int64_t)rows, valid.data());
    make_schema(left_idx_schema, "I", "left_idx", true);
    make_primitive<uint32_t>(right_idx, pi.data(), (int64_t)rows, nullptr);
    make_schema(right_idx_schema, "I", "right_idx", false);
    if (compute_distance && distance) {
        make_primitive<int64_t>(distance, di.data(), (int64_t)rows, valid.data());
        make_schema(distance_schema, "l", "distance", true);
    }
    return 0;
}

namespace {
// brh_interval_join and brh_interval_join_where: where = null is the plain join.  Under a threshold every join type is taken
// from the same filtered matches: Inner = the fill, then ivx_pairs_where; RightSemi / RightAnti from the filtered exists;
// LeftSemi / LeftAnti from the filtered marks; Left / Right / Full = the filtered pairs, then the rows without one.
int interval_join_impl(brh_session *s, brh_batch build, brh_columns bcols, brh_batch probe, brh_columns pcols,
                       int join_type, int strict_predicate, int nearest_algorithm, const brh_overlap_where *where,
                       ArrowArray *build_idx, ArrowSchema *build_idx_schema, ArrowArray *probe_idx, ArrowSchema *probe_idx_schema)
{
    if (!s) return 1;
    if (nearest_algorithm && join_marks_build(join_type)) return fail(s, "interval join: Algorithm::CoitreesNearest is an Inner join");
    const WhereArg wa(where);
    const ivx_overlap_where *w = wa.p;
    if (nearest_algorithm && wa.asks()) return fail(s, "interval join: an overlap threshold (where) does not apply to Algorithm::CoitreesNearest");
    KeyDict kd; Side32 B, P;
    if (build_keys(s, {{build, bcols}, {probe, pcols}}, &kd, true) || load_side32(s, build, bcols, &B) || load_side32(s, probe, pcols, &P)) return 1;
    if (strict_predicate) {                                       // `a.start < b.end AND a.end > b.start`: end - 1 on both sides
        for (auto &v : B.e) v = (int32_t)((uint32_t)v - 1u);
        for (auto &v : P.e) v = (int32_t)((uint32_t)v - 1u);
    }
    const uint32_t nk = (uint32_t)std::max<size_t>(kd.names.size(), 1);
    IndexGuard g;
    ivx_status st = ivx_index_build(s->ctx, nearest_algorithm ? IVX_KIND_NEAREST : IVX_KIND_OVERLAP, IVX_MEM_HOST, kd.ids[0].data(),
                                    B.s.data(), B.e.data(), B.s.size(), nk, &g.ix);
    if (st != IVX_OK) return fail_ivx(s, st);
    const uint64_t np = P.s.size();
    if (nearest_algorithm) {                                      // interval_join.rs:864-870, :1628-1635
        std::vector<uint32_t> bi(np ? np : 1), pi(np ? np : 1);
        uint64_t rows = 0;
        st = ivx_probe_nearest(s->ctx, g.ix, IVX_MEM_HOST, kd.ids[1].data(), P.s.data(), P.e.data(), np, 0, 1, 1, bi.data(), pi.data(), nullptr, np, &rows);
        if (st != IVX_OK) return fail_ivx(s, st);
        std::vector<uint8_t> valid(rows ? rows : 1);
        for (uint64_t i = 0; i < rows; i++) { valid[i] = bi[i] != IVX_NULL_IDX; if (!valid[i]) bi[i] = 0; }
        make_primitive<uint32_t>(build_idx, bi.data(), (int64_t)rows, valid.data()); make_schema(build_idx_schema, "I", "build_idx", true);
        make_primitive<uint32_t>(probe_idx, pi.data(), (int64_t)rows, nullptr); make_schema(probe_idx_schema, "I", "probe_idx", false);
        return 0;
    }
    if (join_type == BRH_JOIN_RIGHT_SEMI || join_type == BRH_JOIN_RIGHT_ANTI) {      // :1014-1024, :1433-1447
        std::vector<uint8_t> ex(np ? np : 1);
        st = probe_exists(s, g.ix, kd.ids[1].data(), P.s.data(), P.e.data(), np, w, ex.data());
        if (st != IVX_OK) return fail_ivx(s, st);
        std::vector<uint32_t> pi;
        const bool want = join_type == BRH_JOIN_RIGHT_SEMI;
        for (uint64_t i = 0; i < np; i++) if ((ex[i] != 0) == want) pi.push_back((uint32_t)i);
        make_primitive<uint32_t>(build_idx, nullptr, 0, nullptr); make_schema(build_idx_schema, "I", "build_idx", false);
        make_primitive<uint32_t>(probe_idx, pi.data(), (int64_t)pi.size(), nullptr); make_schema(probe_idx_schema, "I", "probe_idx", false);
        return 0;
    }
    const uint64_t nb = B.s.size();
    if (join_type == BRH_JOIN_LEFT_SEMI || join_type == BRH_JOIN_LEFT_ANTI) {        // the build rows with / without a match: no pairs are made
        std::vector<uint32_t> marks((nb + 31) / 32 + 1, 0u), rows;
        st = ivx_probe_mark_build_where(s->ctx, g.ix, IVX_MEM_HOST, kd.ids[1].data(), P.s.data(), P.e.data(), np, w, marks.data());
        if (st != IVX_OK) return fail_ivx(s, st);
        if (select_build_rows(s, marks, nb, join_type == BRH_JOIN_LEFT_SEMI, &rows)) return 1;
        make_primitive<uint32_t>(build_idx, rows.data(), (int64_t)rows.size(), nullptr); make_schema(build_idx_schema, "I", "build_idx", false);
        make_primitive<uint32_t>(probe_idx, nullptr, 0, nullptr); make_schema(probe_idx_schema, "I", "probe_idx", false);
        return 0;
    }
    if (join_marks_build(join_type)) {                                               // Left / Right / Full: the pairs, then the NULL-extended rows
        const bool nullb = join_null_build(join_type), nullp = join_null_probe(join_type);
        std::vector<uint32_t> bi, pi; std::vector<uint8_t> bvalid, pvalid;
        uint64_t n_pairs = 0;
        if (join_pairs(s, g.ix, kd.ids[1].data(), P.s.data(), P.e.data(), np, nullb, &bi, &pi, &bvalid, &n_pairs, w, B.s.data(), B.e.data(), nb)) return 1;
        if (nullp) {
            std::vector<uint32_t> marks((nb + 31) / 32 + 1, 0u), rows;
            st = ivx_bits_mark(s->ctx, IVX_MEM_HOST, bi.data(), n_pairs, marks.data(), nb);
            if (st != IVX_OK) return fail_ivx(s, st);
            if (select_build_rows(s, marks, nb, false, &rows)) return 1;
            pvalid.assign(bi.size(), 1);
            for (uint32_t r : rows) { bi.push_back(r); pi.push_back(0u); pvalid.push_back(0); }
            if (nullb) bvalid.resize(bi.size(), 1);
        }
        make_primitive<uint32_t>(build_idx, bi.data(), (int64_t)bi.size(), nullb ? bvalid.data() : nullptr); make_schema(build_idx_schema, "I", "build_idx", nullb);
        make_primitive<uint32_t>(probe_idx, pi.data(), (int64_t)pi.size(), nullp ? pvalid.data() : nullptr); make_schema(probe_idx_schema, "I", "probe_idx", nullp);
        return 0;
    }
    if (w) {                                                                         // Inner under a threshold: the fill, then the pair filter
        std::vector<uint32_t> bi, pi; std::vector<uint8_t> unused;
        uint64_t n_pairs = 0;
        if (join_pairs(s, g.ix, kd.ids[1].data(), P.s.data(), P.e.data(), np, false, &bi, &pi, &unused, &n_pairs, w, B.s.data(), B.e.data(), nb)) return 1;
        make_primitive<uint32_t>(build_idx, bi.data(), (int64_t)n_pairs, nullptr); make_schema(build_idx_schema, "I", "build_idx", false);
        make_primitive<uint32_t>(probe_idx, pi.data(), (int64_t)n_pairs, nullptr); make_schema(probe_idx_schema, "I", "probe_idx", false);
        return 0;
    }
    uint64_t total = 0;
    st = ivx_probe_overlap_count(s->ctx, g.ix, IVX_MEM_HOST, kd.ids[1].data(), P.s.data(), P.e.data(), np, nullptr, &total);
    if (st != IVX_OK) return fail_ivx(s, st);
    std::vector<uint32_t> bi(total ? total : 1), pi(total ? total : 1);
    uint64_t written = 0;
    st = ivx_probe_overlap_fill(s->ctx, g.ix, IVX_MEM_HOST, kd.ids[1].data(), P.s.data(), P.e.data(), np, bi.data(), pi.data(), total, &written);
    if (st != IVX_OK) return fail_ivx(s, st);
    make_primitive<uint32_t>(build_idx, bi.data(), (int64_t)written, nullptr); make_schema(build_idx_schema, "I", "build_idx", false);
    make_primitive<uint32_t>(probe_idx, pi.data(), (int64_t)written, nullptr); make_schema(probe_idx_schema, "I", "probe_idx", false);
    return 0;
}
}  // namespace

extern "C" int brh_interval_join(brh_session *s, brh_batch build, brh_columns bcols, brh_batch probe, brh_columns pcols,
                                 int join_type, int strict_predicate, int nearest_algorithm,
                                 ArrowArray *build_idx, ArrowSchema *build_idx_schema, ArrowArray *probe_idx, ArrowSchema *probe_idx_schema)
{
    return interval_join_impl(s, build, bcols, probe, pcols, join_type, strict_predicate, nearest_algorithm, nullptr,
                              build_idx, build_idx_schema, probe_idx, probe_idx_schema);
}
extern "C" int brh_interval_join_where(brh_session *s, brh_batch build, brh_columns bcols, brh_batch probe, brh_columns pcols,
                                       int join_type, int strict_predicate, int nearest_algorithm, const brh_overlap_where *where,
                                       ArrowArray *build_idx, ArrowSchema *build_idx_schema, ArrowArray *probe_idx, ArrowSchema *probe_idx_schema)
{
    return interval_join_impl(s, build, bcols, probe, pcols, join_type, strict_predicate, nearest_algorithm, where,
                              build_idx, build_idx_schema, probe_idx, probe_idx_schema);
}

// ---- overlap aggregates: join on overlap, group by probe row, aggregate a build-side value (ivx.h ivx_probe_overlap_agg)
namespace {

// the build side's value column, widened to what the device takes: int32 (Int8, Int16, Int32, UInt8, UInt16) or int64
// (UInt32, Int64).  Everything else is refused by name, for the operator `op`
int load_agg_values(brh_session *s, brh_batch t, const char *name, std::vector<int32_t> *v32, std::vector<int64_t> *v64, uint32_t *val_bytes,
                    const std::string &op = "overlap_aggregate")
{
    const int c = find_col(t.schema, name);
    if (c < 0) return fail(s, op + ": value column '" + std::string(name) + "' not found in batch with columns: " + column_list(t.schema));
    const char *f = t.schema->children[c]->format;
    const std::string what = op + ": unsupported data type " + std::string(f) + " for value column '" + name + "'";
    if (!std::strcmp(f, "L")) return fail(s, what + ": UInt64 values do not fit the Int64 aggregates");
    if (!std::strcmp(f, "e") || !std::strcmp(f, "f") || !std::strcmp(f, "g"))
        return fail(s, what + ": float values are not supported (their sums would not be bit-reproducible)");
    if (std::strlen(f) != 1 || !std::strchr("csilCSI", f[0])) return fail(s, what + "; expected Int8, Int16, Int32, Int64, UInt8, UInt16 or UInt32");
    const ArrowArray *a = t.array->children[c];
    if (null_count(a) > 0) return fail(s, op + ": value column '" + std::string(name) + "' contains null values");
    const int64_t n = a->length, o = a->offset;
    const void *d = a->n_buffers >= 2 ? a->buffers[1] : nullptr;
    const bool wide = f[0] == 'l' || f[0] == 'I';
    *val_bytes = wide ? 8u : 4u;
    if (wide) v64->resize((size_t)n); else v32->resize((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        switch (f[0]) {
        case 'c': (*v32)[i] = ((const int8_t *)d)[o + i]; break;
        case 's': (*v32)[i] = ((const int16_t *)d)[o + i]; break;
        case 'i': (*v32)[i] = ((const int32_t *)d)[o + i]; break;
        case 'C': (*v32)[i] = ((const uint8_t *)d)[o + i]; break;
        case 'S': (*v32)[i] = ((const uint16_t *)d)[o + i]; break;
        case 'I': (*v64)[i] = ((const uint32_t *)d)[o + i]; break;
        default: (*v64)[i] = ((const int64_t *)d)[o + i]; break;
        }
    }
    return 0;
}

// overlap select's value column: a selection needs only the values' ORDER, so beside what load_agg_values takes (*exact: the
// int64 the device compares IS the value) it takes UInt64 and Float32 / Float64 through a monotone map into int64 order
// (*exact = false: the caller gets no score, it takes the value with build_idx).  UInt64: the top bit flipped.  Floats:
// widened to double, the bits as int64 i, i ^= INT64_MAX when i < 0 -- the order of the reals with -0.0 below +0.0; a NaN
// has no place in that order and is refused
int load_sel_values(brh_session *s, brh_batch t, const char *name, std::vector<int32_t> *v32, std::vector<int64_t> *v64, uint32_t *val_bytes, bool *exact)
{
    static const std::string op = "overlap_select";
    const int c = find_col(t.schema, name);
    const char *f = c < 0 ? "" : t.schema->children[c]->format;
    *exact = true;
    if (!std::strcmp(f, "e")) return fail(s, op + ": unsupported data type e for value column '" + name + "': Float16 is not supported, cast it to Float32");
    if (std::strcmp(f, "L") && std::strcmp(f, "f") && std::strcmp(f, "g")) return load_agg_values(s, t, name, v32, v64, val_bytes, op);
    const ArrowArray *a = t.array->children[c];
    if (null_count(a) > 0) return fail(s, op + ": value column '" + std::string(name) + "' contains null values");
    const int64_t n = a->length, o = a->offset;
    const void *d = a->n_buffers >= 2 ? a->buffers[1] : nullptr;
    *exact = false;
    *val_bytes = 8u;
    v64->resize((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        if (f[0] == 'L') { (*v64)[i] = (int64_t)(((const uint64_t *)d)[o + i] ^ 0x8000000000000000ull); continue; }
        const double x = f[0] == 'f' ? (double)((const float *)d)[o + i] : ((const double *)d)[o + i];
        if (x != x) return fail(s, op + ": value column '" + std::string(name) + "' contains NaN values");
        int64_t bits;
        std::memcpy(&bits, &x, sizeof bits);
        (*v64)[i] = bits < 0 ? bits ^ INT64_MAX : bits;
    }
    return 0;
}

}  // namespace

// ---- overlap select: join on overlap, keep the one best build row per probe row (ivx_select.h ivx_probe_overlap_select)
static int overlap_select_impl(brh_session *s, brh_batch build, brh_columns bcols, const char *value_column,
                               brh_batch probe, brh_columns pcols, int strict_predicate, int by, const brh_overlap_where *where,
                               ArrowArray *build_idx, ArrowSchema *build_idx_schema, ArrowArray *score, ArrowSchema *score_schema)
{
    if (!s) return 1;
    const WhereArg wa(where);
    if (!build_idx || !build_idx_schema || !score || !score_schema) return fail(s, "overlap_select: null outputs");
    if (by < 0 || by >= BRH_SEL_N) return fail(s, "overlap_select: by is one of the BRH_SEL_* criteria, got " + std::to_string(by));
    const bool by_val = by == BRH_SEL_MIN_VAL || by == BRH_SEL_MAX_VAL;
    if (by_val && !value_column) return fail(s, "overlap_select: the criterion selects by value and no value column is named");
    if (!by_val && value_column) return fail(s, "overlap_select: value column '" + std::string(value_column) + "' given with a criterion that reads no value");
    KeyDict kd; Side32 B, P;
    std::vector<int32_t> v32; std::vector<int64_t> v64; uint32_t vb = 4; bool exact = true;
    if (by_val && load_sel_values(s, build, value_column, &v32, &v64, &vb, &exact)) return 1;
    if (build_keys(s, {{build, bcols}, {probe, pcols}}, &kd, true) || load_side32(s, build, bcols, &B) || load_side32(s, probe, pcols, &P)) return 1;
    if (strict_predicate) {                                       // as brh_interval_join: end - 1 on both sides, and the lengths follow
        for (auto &v : B.e) v = (int32_t)((uint32_t)v - 1u);
        for (auto &v : P.e) v = (int32_t)((uint32_t)v - 1u);
    }
    const uint32_t nk = (uint32_t)std::max<size_t>(kd.names.size(), 1);
    IndexGuard g;
    ivx_status st = ivx_index_build(s->ctx, IVX_KIND_OVERLAP, IVX_MEM_HOST, kd.ids[0].data(), B.s.data(), B.e.data(), B.s.size(), nk, &g.ix);
    if (st != IVX_OK) return fail_ivx(s, st);
    const uint64_t np = P.s.size(), na = np ? np : 1;
    std::vector<uint32_t> bi(na);
    std::vector<int64_t> sc(exact ? na : 0);
    const void *val = !by_val ? nullptr : vb == 4 ? (const void *)v32.data() : (const void *)v64.data();     // (may be null for an empty build side: never read)
    st = ivx_probe_overlap_select_where(s->ctx, g.ix, IVX_MEM_HOST, kd.ids[1].data(), P.s.data(), P.e.data(), np, val, vb, by, wa.p,
                                        bi.data(), exact ? sc.data() : nullptr);
    if (st != IVX_OK) return fail_ivx(s, st);
    std::vector<uint8_t> valid(na);
    for (uint64_t i = 0; i < np; i++) { valid[i] = bi[i] != IVX_NULL_IDX; if (!valid[i]) bi[i] = 0; }     // (a NULL slot's value)
    make_primitive<uint32_t>(build_idx, bi.data(), (int64_t)np, valid.data()); make_schema(build_idx_schema, "I", "build_idx", true);
    std::memset(score, 0, sizeof *score); std::memset(score_schema, 0, sizeof *score_schema);
    if (exact) { make_primitive<int64_t>(score, sc.data(), (int64_t)np, valid.data()); make_schema(score_schema, "l", "score", true); }
    return 0;
}
extern "C" int brh_overlap_select(brh_session *s, brh_batch build, brh_columns bcols, const char *value_column,
                                  brh_batch probe, brh_columns pcols, int strict_predicate, int by,
                                  ArrowArray *build_idx, ArrowSchema *build_idx_schema, ArrowArray *score, ArrowSchema *score_schema)
{
    return overlap_select_impl(s, build, bcols, value_column, probe, pcols, strict_predicate, by, nullptr, build_idx, build_idx_schema, score, score_schema);
}
extern "C" int brh_overlap_select_where(brh_session *s, brh_batch build, brh_columns bcols, const char *value_column,
                                        brh_batch probe, brh_columns pcols, int strict_predicate, int by, const brh_overlap_where *where,
                                        ArrowArray *build_idx, ArrowSchema *build_idx_schema, ArrowArray *score, ArrowSchema *score_schema)
{
    return overlap_select_impl(s, build, bcols, value_column, probe, pcols, strict_predicate, by, where, build_idx, build_idx_schema, score, score_schema);
}

static int overlap_aggregate_impl(brh_session *s, brh_batch build, brh_columns bcols, const char *value_column,
                                  brh_batch probe, brh_columns pcols, int strict_predicate, uint32_t ops, const brh_overlap_where *where,
                                  ArrowArray *out, ArrowSchema *out_schema)
{
    if (!s) return 1;
    const WhereArg wa(where);
    if (!value_column) return fail(s, "overlap_aggregate: null value column name");
    if (!out || !out_schema) return fail(s, "overlap_aggregate: null outputs");
    if (ops == 0 || (ops & ~(uint32_t)BRH_AGG_ALL)) return fail(s, "overlap_aggregate: ops is a non-empty set of BRH_AGG_* bits");
    KeyDict kd; Side32 B, P;
    std::vector<int32_t> v32; std::vector<int64_t> v64; uint32_t vb = 4;
    if (load_agg_values(s, build, value_column, &v32, &v64, &vb)) return 1;
    if (build_keys(s, {{build, bcols}, {probe, pcols}}, &kd, true) || load_side32(s, build, bcols, &B) || load_side32(s, probe, pcols, &P)) return 1;
    if (strict_predicate) {                                       // as brh_interval_join: end - 1 on both sides, and the lengths follow
        for (auto &v : B.e) v = (int32_t)((uint32_t)v - 1u);
        for (auto &v : P.e) v = (int32_t)((uint32_t)v - 1u);
    }
    const uint32_t nk = (uint32_t)std::max<size_t>(kd.names.size(), 1);
    IndexGuard g;
    ivx_status st = ivx_index_build(s->ctx, IVX_KIND_OVERLAP, IVX_MEM_HOST, kd.ids[0].data(), B.s.data(), B.e.data(), B.s.size(), nk, &g.ix);
    if (st != IVX_OK) return fail_ivx(s, st);
    const uint64_t np = P.s.size(), na = np ? np : 1;
    // the count says where sum / min / max / wsum are NULL: fetched whenever one of them is wanted
    const bool nullable = (ops & (BRH_AGG_SUM | BRH_AGG_MIN | BRH_AGG_MAX | BRH_AGG_WSUM)) != 0;
    std::vector<uint32_t> cnt((ops & BRH_AGG_COUNT) || nullable ? na : 0);
    std::vector<int64_t> col[BRH_AGG_N];
    for (int k = 1; k < BRH_AGG_N; k++) if (ops & (1u << k)) col[k].resize(na);
    auto ptr = [&](int k) { return col[k].empty() ? nullptr : col[k].data(); };
    const void *val = vb == 4 ? (const void *)v32.data() : (const void *)v64.data();     // (may be null for an empty build side: never read)
    st = ivx_probe_overlap_agg_where(s->ctx, g.ix, IVX_MEM_HOST, kd.ids[1].data(), P.s.data(), P.e.data(), np, val, vb, wa.p,
                                     cnt.empty() ? nullptr : cnt.data(), ptr(1), ptr(2), ptr(3), ptr(4), ptr(5));
    if (st != IVX_OK) return fail_ivx(s, st);
    std::vector<uint8_t> valid(nullable ? na : 0);
    for (uint64_t i = 0; nullable && i < np; i++) valid[i] = cnt[i] != 0;
    static const char *const names[BRH_AGG_N] = {"count", "sum", "min", "max", "bases", "wsum"};
    for (int k = 0; k < BRH_AGG_N; k++) {
        std::memset(&out[k], 0, sizeof out[k]); std::memset(&out_schema[k], 0, sizeof out_schema[k]);
        if (!(ops & (1u << k))) continue;
        const bool nulls = k != 0 && k != 4;                      // count and bases: 0 without a match; the others NULL, as SQL over a left join
        if (k == 0) { col[0].resize(na); for (uint64_t i = 0; i < np; i++) col[0][i] = (int64_t)cnt[i]; }
        else if (nulls) for (uint64_t i = 0; i < np; i++) if (!valid[i]) col[k][i] = 0;     // (a NULL slot's value)
        make_primitive<int64_t>(&out[k], col[k].data(), (int64_t)np, nulls ? valid.data() : nullptr);
        make_schema(&out_schema[k], "l", names[k], nulls);
    }
    return 0;
}
extern "C" int brh_overlap_aggregate(brh_session *s, brh_batch build, brh_columns bcols, const char *value_column,
                                     brh_batch probe, brh_columns pcols, int strict_predicate, uint32_t ops,
                                     ArrowArray *out, ArrowSchema *out_schema)
{
    return overlap_aggregate_impl(s, build, bcols, value_column, probe, pcols, strict_predicate, ops, nullptr, out, out_schema);
}
extern "C" int brh_overlap_aggregate_where(brh_session *s, brh_batch build, brh_columns bcols, const char *value_column,
                                           brh_batch probe, brh_columns pcols, int strict_predicate, uint32_t ops, const brh_overlap_where *where,
                                           ArrowArray *out, ArrowSchema *out_schema)
{
    return overlap_aggregate_impl(s, build, bcols, value_column, probe, pcols, strict_predicate, ops, where, out, out_schema);
}

extern "C" int brh_merge(brh_session *s, brh_batch table, brh_columns cols, int64_t min_dist, int filter_op,
                         ArrowArray *contig, ArrowSchema *contig_schema, ArrowArray *start, ArrowSchema *start_schema,
                         ArrowArray *end, ArrowSchema *end_schema, ArrowArray *n_intervals, ArrowSchema *n_schema)
{
    if (!s) return 1;
    KeyDict kd; Side64 T;
    if (build_keys(s, {{table, cols}}, &kd) || load_side64(s, table, cols, &T)) return 1;
    const uint64_t n = T.s.size();
    std::vector<uint32_t> ok(n ? n : 1); std::vector<int64_t> os(n ? n : 1), oe(n ? n : 1), on(n ? n : 1);
    uint64_t m = 0;
    ivx_status st = ivx_merge(s->ctx, IVX_MEM_HOST, kd.ids[0].data(), T.s.data(), T.e.data(), n, (uint32_t)std::max<size_t>(kd.names.size(), 1),
                              min_dist, filter_op == BRH_STRICT, ok.data(), os.data(), oe.data(), on.data(), n, &m);
    if (st != IVX_OK) return fail_ivx(s, st);
    make_utf8(contig, kd.names, ok.data(), (int64_t)m); make_schema(contig_schema, "u", cols.keys[0], false);
    make_primitive<int64_t>(start, os.data(), (int64_t)m, nullptr); make_schema(start_schema, "l", cols.start, false);   // merge.rs:43-48
    make_primitive<int64_t>(end, oe.data(), (int64_t)m, nullptr); make_schema(end_schema, "l", cols.end, false);
    make_primitive<int64_t>(n_intervals, on.data(), (int64_t)m, nullptr); make_schema(n_schema, "l", "n_intervals", false);
    return 0;
}

// subtract and intersect: the same arguments, the same sizing-then-fill protocol, the same schema (the left table's names)
static int left_pieces(decltype(&ivx_subtract) op, brh_session *s, brh_batch left, brh_columns lcols, brh_batch right, brh_columns rcols, int filter_op,
                       ArrowArray *contig, ArrowSchema *contig_schema, ArrowArray *start, ArrowSchema *start_schema,
                       ArrowArray *end, ArrowSchema *end_schema, ArrowArray *left_row, ArrowSchema *left_row_schema)
{
    if (!s) return 1;
    KeyDict kd; Side64 L, R;
    if (build_keys(s, {{left, lcols}, {right, rcols}}, &kd) || load_side64(s, left, lcols, &L) || load_side64(s, right, rcols, &R)) return 1;
    const uint32_t nk = (uint32_t)std::max<size_t>(kd.names.size(), 1);
    uint64_t m = 0, m2 = 0;                              // sizing call, then the fill call
    ivx_status st = op(s->ctx, IVX_MEM_HOST, kd.ids[0].data(), L.s.data(), L.e.data(), L.s.size(), kd.ids[1].data(), R.s.data(), R.e.data(),
                       R.s.size(), nk, filter_op == BRH_STRICT, nullptr, nullptr, nullptr, nullptr, 0, &m);
    if (st != IVX_OK) return fail_ivx(s, st);
    std::vector<uint32_t> ok(m ? m : 1), orow(m ? m : 1); std::vector<int64_t> os(m ? m : 1), oe(m ? m : 1);
    st = op(s->ctx, IVX_MEM_HOST, kd.ids[0].data(), L.s.data(), L.e.data(), L.s.size(), kd.ids[1].data(), R.s.data(), R.e.data(),
            R.s.size(), nk, filter_op == BRH_STRICT, ok.data(), os.data(), oe.data(), orow.data(), m, &m2);
    if (st != IVX_OK) return fail_ivx(s, st);
    make_utf8(contig, kd.names, ok.data(), (int64_t)m2); make_schema(contig_schema, "u", lcols.keys[0], false);
    make_primitive<int64_t>(start, os.data(), (int64_t)m2, nullptr); make_schema(start_schema, "l", lcols.start, false);   // subtract.rs:57-72
    make_primitive<int64_t>(end, oe.data(), (int64_t)m2, nullptr); make_schema(end_schema, "l", lcols.end, false);
    make_primitive<uint32_t>(left_row, orow.data(), (int64_t)m2, nullptr); make_schema(left_row_schema, "I", "left_row", false);
    return 0;
}

extern "C" int brh_subtract(brh_session *s, brh_batch left, brh_columns lcols, brh_batch right, brh_columns rcols, int filter_op,
                            ArrowArray *contig, ArrowSchema *contig_schema, ArrowArray *start, ArrowSchema *start_schema,
                            ArrowArray *end, ArrowSchema *end_schema, ArrowArray *left_row, ArrowSchema *left_row_schema)
{
    return left_pieces(ivx_subtract, s, left, lcols, right, rcols, filter_op, contig, contig_schema, start, start_schema, end, end_schema, left_row, left_row_schema);
}

extern "C" int brh_intersect(brh_session *s, brh_batch left, brh_columns lcols, brh_batch right, brh_columns rcols, int filter_op,
                             ArrowArray *contig, ArrowSchema *contig_schema, ArrowArray *start, ArrowSchema *start_schema,
                             ArrowArray *end, ArrowSchema *end_schema, ArrowArray *left_row, ArrowSchema *left_row_schema)
{
    return left_pieces(ivx_intersect, s, left, lcols, right, rcols, filter_op, contig, contig_schema, start, start_schema, end, end_schema, left_row, left_row_schema);
}

extern "C" int brh_cluster(brh_session *s, brh_batch table, brh_columns cols, int64_t min_dist, int filter_op,
                           ArrowArray *contig, ArrowSchema *contig_schema, ArrowArray *start, ArrowSchema *start_schema,
                           ArrowArray *end, ArrowSchema *end_schema, ArrowArray *row, ArrowSchema *row_schema,
                           ArrowArray *cluster, ArrowSchema *cluster_schema, ArrowArray *cluster_start, ArrowSchema *cluster_start_schema,
                           ArrowArray *cluster_end, ArrowSchema *cluster_end_schema)
{
    if (!s) return 1;
    KeyDict kd; Side64 T;
    if (build_keys(s, {{table, cols}}, &kd) || load_side64(s, table, cols, &T)) return 1;
    const uint64_t n = T.s.size(), na = n ? n : 1;
    std::vector<uint32_t> ok(na), orow(na); std::vector<int64_t> os(na), oe(na), oc(na), ocs(na), oce(na);
    uint64_t m = 0;
    ivx_status st = ivx_cluster(s->ctx, IVX_MEM_HOST, kd.ids[0].data(), T.s.data(), T.e.data(), n, (uint32_t)std::max<size_t>(kd.names.size(), 1),
                                min_dist, filter_op == BRH_STRICT, nullptr, ok.data(), os.data(), oe.data(), orow.data(),
                                oc.data(), ocs.data(), oce.data(), nullptr, &m);
    if (st != IVX_OK) return fail_ivx(s, st);
    make_utf8(contig, kd.names, ok.data(), (int64_t)n); make_schema(contig_schema, "u", cols.keys[0], false);
    make_primitive<int64_t>(start, os.data(), (int64_t)n, nullptr); make_schema(start_schema, "l", cols.start, false);   // cluster.rs:55-67
    make_primitive<int64_t>(end, oe.data(), (int64_t)n, nullptr); make_schema(end_schema, "l", cols.end, false);
    make_primitive<uint32_t>(row, orow.data(), (int64_t)n, nullptr); make_schema(row_schema, "I", "row", false);
    make_primitive<int64_t>(cluster, oc.data(), (int64_t)n, nullptr); make_schema(cluster_schema, "l", "cluster", false);
    make_primitive<int64_t>(cluster_start, ocs.data(), (int64_t)n, nullptr); make_schema(cluster_start_schema, "l", "cluster_start", false);
    make_primitive<int64_t>(cluster_end, oce.data(), (int64_t)n, nullptr); make_schema(cluster_end_schema, "l", "cluster_end", false);
    return 0;
}

extern "C" int brh_complement(brh_session *s, brh_batch table, brh_columns cols, brh_batch view, brh_columns view_cols, int filter_op,
                              ArrowArray *contig, ArrowSchema *contig_schema, ArrowArray *start, ArrowSchema *start_schema,
                              ArrowArray *end, ArrowSchema *end_schema)
{
    if (!s) return 1;
    const bool has_view = view.array != nullptr;
    KeyDict kd; Side64 T, V;
    if (has_view) {
        if (build_keys(s, {{table, cols}, {view, view_cols}}, &kd) || load_side64(s, table, cols, &T) || load_side64(s, view, view_cols, &V)) return 1;
    } else {
        if (build_keys(s, {{table, cols}}, &kd) || load_side64(s, table, cols, &T)) return 1;
        kd.ids.emplace_back();
    }
    const uint32_t nk = (uint32_t)std::max<size_t>(kd.names.size(), 1);
    const bool strict = filter_op == BRH_STRICT;
    uint64_t m = T.s.size() + 2 * V.s.size() + 2 * (uint64_t)nk + 16, m2 = 0;
    std::vector<uint32_t> ok(m); std::vector<int64_t> os(m), oe(m);
    ivx_status st = ivx_complement(s->ctx, IVX_MEM_HOST, kd.ids[0].data(), T.s.data(), T.e.data(), T.s.size(),
                                   kd.ids[1].data(), V.s.data(), V.e.data(), V.s.size(), nk, strict, ok.data(), os.data(), oe.data(), m, &m2);
    if (st == IVX_ERR_CAPACITY) {                        // heavily overlapping views: repeat with the exact size
        m = m2 ? m2 : 1;
        ok.resize(m); os.resize(m); oe.resize(m);
        st = ivx_complement(s->ctx, IVX_MEM_HOST, kd.ids[0].data(), T.s.data(), T.e.data(), T.s.size(),
                            kd.ids[1].data(), V.s.data(), V.e.data(), V.s.size(), nk, strict, ok.data(), os.data(), oe.data(), m, &m2);
    }
    if (st != IVX_OK) return fail_ivx(s, st);
    make_utf8(contig, kd.names, ok.data(), (int64_t)m2); make_schema(contig_schema, "u", cols.keys[0], false);           // complement.rs:52-58
    make_primitive<int64_t>(start, os.data(), (int64_t)m2, nullptr); make_schema(start_schema, "l", cols.start, false);
    make_primitive<int64_t>(end, oe.data(), (int64_t)m2, nullptr); make_schema(end_schema, "l", cols.end, false);
    return 0;
}

// ---- depth(): the pileup crate's coverage blocks (bio-function-pileup process_batch* + *_to_coverage_blocks)
namespace {

// a UInt32 column of the reads batch (schema.rs:7-11); the validity of flags / mapping_quality is not read, as in the reference
int get_u32(brh_session *s, brh_batch t, const char *name, const ArrowArray **out)
{
    const int c = find_col(t.schema, name);
    if (c < 0) return fail(s, "depth: column '" + std::string(name) + "' not found in batch with columns: " + column_list(t.schema));
    if (std::strcmp(t.schema->children[c]->format, "I"))
        return fail(s, "depth: unsupported data type " + std::string(t.schema->children[c]->format) + " for column '" + name + "'; expected UInt32");
    *out = t.array->children[c];
    return 0;
}

bool slot_null(const ArrowArray *a, int64_t i)
{
    if (a->n_buffers < 1 || !a->buffers[0] || a->null_count == 0) return false;
    const uint8_t *v = (const uint8_t *)a->buffers[0];
    const int64_t j = i + a->offset;
    return !((v[j >> 3] >> (j & 7)) & 1);
}

// contig names -> ids in byte order (both of the reference's modes sort their contigs: coverage.rs:75-76,
// physical_exec.rs:400-402); id_of gives IVX_NULL_IDX for a name the dictionary lacks
struct NameDict {
    std::vector<std::string> names;
    std::unordered_map<std::string_view, uint32_t> ids;
    void finish(std::vector<std::string_view> &uniq)
    {
        std::sort(uniq.begin(), uniq.end());
        uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
        names.assign(uniq.begin(), uniq.end());
        for (uint32_t i = 0; i < names.size(); i++) ids.emplace(std::string_view(names[i]), i);
    }
    uint32_t id_of(std::string_view k) const { auto it = ids.find(k); return it == ids.end() ? IVX_NULL_IDX : it->second; }
};

void collect_names(const StrCol &c, std::vector<std::string_view> *uniq)
{
    std::string_view last; bool have = false;
    for (int64_t i = 0; i < c.a->length; i++) {
        if (c.null_at(i)) continue;
        const std::string_view k = c.at(i);
        if (have && k == last) continue;
        last = k; have = true;
        uniq->push_back(k);
    }
}

void ids_of(const StrCol &c, const NameDict &d, std::vector<uint32_t> *out)
{
    out->resize((size_t)c.a->length);
    std::string_view last; uint32_t last_id = IVX_NULL_IDX; bool have = false;
    for (int64_t i = 0; i < c.a->length; i++) {
        if (c.null_at(i)) { (*out)[i] = IVX_NULL_IDX; continue; }
        const std::string_view k = c.at(i);
        if (!have || k != last) { last_id = d.id_of(k); last = k; have = true; }
        (*out)[i] = last_id;
    }
}

// the length table (name Utf8, length: any integer type, clamped to [0, 2^32-1]) -> its contigs in byte order and their lengths
// (at least one slot: key 0 stands for no contig when the table is empty)
int load_lengths(brh_session *s, brh_batch lengths, NameDict *dict, std::vector<uint32_t> *key_len)
{
    StrCol lname; PosCol pl;
    std::vector<int64_t> len64;
    if (get_contig(s, lengths, "name", &lname) || get_pos(s, lengths, "length", "length", &pl) || resolve_i64(s, pl, &len64)) return 1;
    std::vector<std::string_view> uniq;
    collect_names(lname, &uniq);
    dict->finish(uniq);
    key_len->assign(std::max<size_t>(dict->names.size(), 1), 0);
    for (int64_t i = 0; i < lname.a->length; i++) {
        if (lname.null_at(i)) continue;
        const uint32_t k = dict->id_of(lname.at(i));
        const int64_t v = len64[(size_t)i];
        (*key_len)[k] = v < 0 ? 0u : (v > (int64_t)UINT32_MAX ? UINT32_MAX : (uint32_t)v);
    }
    return 0;
}

}  // namespace

namespace {

// the inputs of one depth() call as ivx_depth / ivx_depth_profile_build take them.  The read columns point into the caller's
// batch: use them before the call that brought the batch returns.
struct DepthInputs {
    bool has_prior = false, has_len = false;
    uint64_t n_reads = 0, n_seg = 0;
    uint32_t nk = 1;
    NameDict dict;
    std::vector<uint32_t> rkey, skey, ss, se, key_len;
    std::vector<int32_t> sw;
    const uint32_t *rpos = nullptr, *rflags = nullptr, *rmapq = nullptr, *cops = nullptr;
    const int32_t *coff = nullptr;
    // a text cigar column (brh_session_set_string_cigars): its offsets (int32, or int64 when large) and bytes instead of coff / cops
    bool text = false; int large = 0;
    const void *toff = nullptr; const uint8_t *ctext = nullptr;
    int load(brh_session *s, brh_batch reads, brh_batch prior, brh_batch lengths);
    // what goes with the read columns: the prior segments and the keys.  own(): this call's; of_stream(): a push stream's keys and
    // length table, no prior segments (its batches carry the stream's ids)
    struct Rest { const uint32_t *skey, *ss, *se; const int32_t *sw; uint64_t n_seg; uint32_t nk; const uint32_t *key_len; };
    Rest own() const
    {
        return Rest{has_prior ? skey.data() : nullptr, ss.data(), se.data(), has_prior ? sw.data() : nullptr, n_seg, nk, has_len ? key_len.data() : nullptr};
    }
    static Rest of_stream(uint32_t nk, const uint32_t *key_len) { return Rest{nullptr, nullptr, nullptr, nullptr, 0, nk, key_len}; }
    // ivx_depth / ivx_depth_text and ivx_depth_profile_build / ..._text on the read columns, whichever form the cigar column has
    ivx_status depth(ivx_ctx *ctx, uint32_t filter_flag, uint32_t min_mapq, uint32_t *ok, uint32_t *os, uint32_t *oe, int32_t *oc, uint64_t cap, uint64_t *m) const
    {
        const Rest r = own();
        if (text)
            return ivx_depth_text(ctx, IVX_MEM_HOST, rkey.data(), rpos, rflags, rmapq, large, toff, ctext, n_reads, r.skey, r.ss, r.se, r.sw, r.n_seg,
                                  r.nk, r.key_len, filter_flag, min_mapq, ok, os, oe, oc, cap, m);
        return ivx_depth(ctx, IVX_MEM_HOST, rkey.data(), rpos, rflags, rmapq, coff, cops, n_reads, r.skey, r.ss, r.se, r.sw, r.n_seg,
                         r.nk, r.key_len, filter_flag, min_mapq, ok, os, oe, oc, cap, m);
    }
    ivx_status profile(ivx_ctx *ctx, uint32_t filter_flag, uint32_t min_mapq, ivx_index **out) const { return profile(ctx, own(), filter_flag, min_mapq, out); }
    ivx_status profile(ivx_ctx *ctx, const Rest &r, uint32_t filter_flag, uint32_t min_mapq, ivx_index **out) const
    {
        if (text)
            return ivx_depth_profile_build_text(ctx, IVX_MEM_HOST, rkey.data(), rpos, rflags, rmapq, large, toff, ctext, n_reads,
                                                r.skey, r.ss, r.se, r.sw, r.n_seg, r.nk, r.key_len, filter_flag, min_mapq, out);
        return ivx_depth_profile_build(ctx, IVX_MEM_HOST, rkey.data(), rpos, rflags, rmapq, coff, cops, n_reads,
                                       r.skey, r.ss, r.se, r.sw, r.n_seg, r.nk, r.key_len, filter_flag, min_mapq, out);
    }
};

// Which profile a statistic reads, and what it needs to know about its keys: the same for a one-shot call (the profile of its
// inputs, owned here) and for a push stream (everything pushed so far, merged; the stream keeps it).
struct ProfileSource {
    const ivx_index *profile = nullptr;
    uint32_t nk = 1, known = 0;                         // keys of the profile; ids below `known` name a contig (an empty dictionary: none)
    const std::vector<std::string> *names = nullptr;    // key id -> contig
    const std::vector<uint32_t> *key_len = nullptr;     // null: no length table
    bool by_name = false;                               // rows go out in byte order of the names, not in id order
    DepthInputs in; IndexGuard g;                       // one-shot
    const brh_depth_push *dp = nullptr;                 // push
    int open(brh_session *s, brh_batch reads, brh_batch prior, brh_batch lengths, uint32_t filter_flag, uint32_t min_mapq)
    {
        if (in.load(s, reads, prior, lengths)) return 1;
        const ivx_status st = in.profile(s->ctx, filter_flag, min_mapq, &g.ix);
        if (st != IVX_OK) return fail_ivx(s, st);
        profile = g.ix; nk = in.nk; known = (uint32_t)in.dict.names.size();
        names = &in.dict.names; key_len = in.has_len ? &in.key_len : nullptr;
        return 0;
    }
    int open(brh_depth_push *dp);                       // depth_push_check + depth_push_merge_all: the merged profile stays the stack's only entry
    uint32_t id_of(std::string_view name) const;        // IVX_NULL_IDX: a contig the source does not know
};

int DepthInputs::load(brh_session *s, brh_batch reads, brh_batch prior, brh_batch lengths)
{
    if (!reads.array || !reads.schema) return fail(s, "depth: null reads batch");
    has_prior = prior.array != nullptr; has_len = lengths.array != nullptr;
    // ---- the reads batch (events.rs:106-112)
    StrCol chrom;
    const ArrowArray *start, *flags, *mapq;
    if (get_contig(s, reads, "chrom", &chrom) || get_u32(s, reads, "start", &start) || get_u32(s, reads, "flags", &flags) ||
        get_u32(s, reads, "mapping_quality", &mapq)) return 1;
    const int cc = find_col(reads.schema, "cigar");
    if (cc < 0) return fail(s, "depth: column 'cigar' not found in batch with columns: " + column_list(reads.schema));
    const char *cf = reads.schema->children[cc]->format;
    const bool is_str = !std::strcmp(cf, "u") || !std::strcmp(cf, "U");
    if (s->string_cigars) {
        if (!is_str && std::strcmp(cf, "z"))
            return fail(s, "depth: unsupported data type " + std::string(cf) + " for column 'cigar'; expected Binary, Utf8 or LargeUtf8");
        text = is_str; large = cf[0] == 'U';
    } else {
        if (is_str || !std::strcmp(cf, "vu"))
            return fail(s, "depth: string CIGAR columns are not supported, use the binary CIGAR column");
        if (std::strcmp(cf, "z")) return fail(s, "depth: unsupported data type " + std::string(cf) + " for column 'cigar'; expected Binary");
    }
    const ArrowArray *cigar = reads.array->children[cc];
    n_reads = (uint64_t)reads.array->length;
    // ---- prior blocks (the output of an earlier call) and the length table
    StrCol pcontig;
    const ArrowArray *pstart = nullptr, *pend = nullptr, *pcov = nullptr;
    char pcov_fmt = 0;
    n_seg = 0;
    if (has_prior) {
        if (get_contig(s, prior, "contig", &pcontig)) return 1;
        const char *names[3] = {"pos_start", "pos_end", "coverage"};
        const ArrowArray **outp[3] = {&pstart, &pend, &pcov};
        for (int k = 0; k < 3; k++) {
            const int c = find_col(prior.schema, names[k]);
            if (c < 0) return fail(s, "depth: column '" + std::string(names[k]) + "' not found in the prior batch with columns: " + column_list(prior.schema));
            const char *f = prior.schema->children[c]->format;
            const bool ok = k < 2 ? (!std::strcmp(f, "i") || !std::strcmp(f, "I")) : (!std::strcmp(f, "s") || !std::strcmp(f, "i"));
            if (!ok) return fail(s, "depth: unsupported data type " + std::string(f) + " for column '" + names[k] + "' of the prior batch; expected " + (k < 2 ? "Int32" : "Int16"));
            if (k == 2) pcov_fmt = f[0];
            *outp[k] = prior.array->children[c];
        }
        n_seg = (uint64_t)prior.array->length;
    }
    // ---- contig ids.  With a length table only its contigs exist: reads (and prior blocks) elsewhere are skipped (events.rs:247-260)
    if (has_len) { if (load_lengths(s, lengths, &dict, &key_len)) return 1; }
    else {
        std::vector<std::string_view> uniq;
        collect_names(chrom, &uniq); if (has_prior) collect_names(pcontig, &uniq);
        dict.finish(uniq);
    }
    nk = (uint32_t)std::max<size_t>(dict.names.size(), 1);
    ids_of(chrom, dict, &rkey);
    for (uint64_t i = 0; i < n_reads; i++) if (slot_null(start, (int64_t)i)) rkey[i] = IVX_NULL_IDX;       // events.rs:114
    if (has_prior) {
        ids_of(pcontig, dict, &skey);
        ss.resize(n_seg); se.resize(n_seg); sw.resize(n_seg);
        for (uint64_t j = 0; j < n_seg; j++) {
            ss[j] = ((const uint32_t *)pstart->buffers[1])[pstart->offset + j];            // Int32 positions are the u32's bits (`as i32`)
            se[j] = ((const uint32_t *)pend->buffers[1])[pend->offset + j];
            sw[j] = pcov_fmt == 's' ? (int32_t)((const int16_t *)pcov->buffers[1])[pcov->offset + j] : ((const int32_t *)pcov->buffers[1])[pcov->offset + j];
        }
    }
    rpos = n_reads ? (const uint32_t *)start->buffers[1] + start->offset : nullptr;
    rflags = n_reads ? (const uint32_t *)flags->buffers[1] + flags->offset : nullptr;
    rmapq = n_reads ? (const uint32_t *)mapq->buffers[1] + mapq->offset : nullptr;
    if (text) {                                              // (the validity of cigar is not read: the reference's schema has it non-null)
        toff = !n_reads ? nullptr : large ? (const void *)((const int64_t *)cigar->buffers[1] + cigar->offset)
                                          : (const void *)((const int32_t *)cigar->buffers[1] + cigar->offset);
        ctext = n_reads ? (const uint8_t *)cigar->buffers[2] : nullptr;
    } else {
        coff = n_reads ? (const int32_t *)cigar->buffers[1] + cigar->offset : nullptr;
        cops = n_reads ? (const uint32_t *)cigar->buffers[2] : nullptr;
    }
    return 0;
}

}  // namespace

extern "C" int brh_depth(brh_session *s, brh_batch reads, brh_batch prior, brh_batch lengths, uint32_t filter_flag, uint32_t min_mapq,
                         ArrowArray *contig, ArrowSchema *contig_schema, ArrowArray *pos_start, ArrowSchema *pos_start_schema,
                         ArrowArray *pos_end, ArrowSchema *pos_end_schema, ArrowArray *coverage, ArrowSchema *coverage_schema)
{
    if (!s) return 1;
    DepthInputs in;
    if (in.load(s, reads, prior, lengths)) return 1;
    // ---- sizing call, then the fill call
    uint64_t m = 0, m2 = 0;
    ivx_status st = in.depth(s->ctx, filter_flag, min_mapq, nullptr, nullptr, nullptr, nullptr, 0, &m);
    if (st != IVX_OK) return fail_ivx(s, st);
    std::vector<uint32_t> ok(m ? m : 1), os(m ? m : 1), oe(m ? m : 1); std::vector<int32_t> oc(m ? m : 1);
    if (m) {
        st = in.depth(s->ctx, filter_flag, min_mapq, ok.data(), os.data(), oe.data(), oc.data(), m, &m2);
        if (st != IVX_OK) return fail_ivx(s, st);
    }
    // ---- schema.rs:28-41: contig Utf8, pos_start / pos_end Int32 (`as i32`), coverage Int16 (`as i16`)
    std::vector<int32_t> o32s(m2 ? m2 : 1), o32e(m2 ? m2 : 1); std::vector<int16_t> o16(m2 ? m2 : 1);
    for (uint64_t i = 0; i < m2; i++) { o32s[i] = (int32_t)os[i]; o32e[i] = (int32_t)oe[i]; o16[i] = (int16_t)oc[i]; }
    make_utf8(contig, in.dict.names, ok.data(), (int64_t)m2); make_schema(contig_schema, "u", "contig", true);
    make_primitive<int32_t>(pos_start, o32s.data(), (int64_t)m2, nullptr); make_schema(pos_start_schema, "i", "pos_start", false);
    make_primitive<int32_t>(pos_end, o32e.data(), (int64_t)m2, nullptr); make_schema(pos_end_schema, "i", "pos_end", false);
    make_primitive<int16_t>(coverage, o16.data(), (int64_t)m2, nullptr); make_schema(coverage_schema, "s", "coverage", false);
    return 0;
}

// ---- depth(per_base = true): the reference's PerBaseEmitter (coverage.rs:271-365) as a pull stream over ONE depth profile
struct brh_depth_stream {
    brh_session *s = nullptr;
    ivx_index *profile = nullptr;
    std::vector<std::string> names;         // contigs in byte order = key ids
    std::vector<uint32_t> key_len;
    std::vector<uint8_t> seen;
    int zero_based = 0;
    uint32_t key = 0;                       // the contig being emitted
    uint64_t next = 0;                      // rows of it already returned
};

extern "C" int brh_depth_per_base_open(brh_session *s, brh_batch reads, brh_batch prior, brh_batch lengths, int zero_based,
                                       uint32_t filter_flag, uint32_t min_mapq, brh_depth_stream **out)
{
    if (!s) return 1;
    if (!out) return fail(s, "depth_per_base: null out");
    *out = nullptr;
    if (!lengths.array)                     // physical_exec.rs:299-303
        return fail(s, "per_base mode requires dense accumulation (BAM header with contig lengths). "
                       "Sparse fallback (e.g. MemTable) is not supported for per_base output.");
    ProfileSource src;
    if (src.open(s, reads, prior, lengths, filter_flag, min_mapq)) return 1;
    std::unique_ptr<brh_depth_stream> ds(new brh_depth_stream());
    ds->s = s; ds->zero_based = zero_based != 0;
    ds->names = *src.names; ds->key_len = *src.key_len;
    ds->seen.assign(src.nk, 0);
    uint64_t steps = 0;
    const ivx_status st = ivx_depth_profile_read(s->ctx, src.profile, IVX_MEM_HOST, nullptr, nullptr, nullptr, ds->seen.data(), 0, &steps);
    if (st != IVX_OK) return fail_ivx(s, st);
    if (ds->names.empty()) ds->seen.assign(ds->seen.size(), 0);     // (an empty length table: key 0 stands for no contig)
    ds->profile = src.g.ix; src.g.ix = nullptr;                     // the profile moves into the pull stream
    *out = ds.release();
    return 0;
}

extern "C" int brh_depth_per_base_next(brh_depth_stream *ds, uint64_t max_rows, int *done,
                                       ArrowArray *contig, ArrowSchema *contig_schema, ArrowArray *pos, ArrowSchema *pos_schema,
                                       ArrowArray *coverage, ArrowSchema *coverage_schema)
{
    if (!ds) return 1;
    brh_session *s = ds->s;
    if (!done) return fail(s, "depth_per_base: null done");
    *done = 0;
    if (max_rows == 0) return fail(s, "depth_per_base: max_rows must be at least 1");
    // the next contig that was touched and still has rows (coverage.rs:319-321)
    while (ds->key < ds->seen.size() && (!ds->seen[ds->key] || ds->next >= ds->key_len[ds->key])) { ds->key++; ds->next = 0; }
    if (ds->key >= ds->seen.size()) { *done = 1; return 0; }
    const std::string &name = ds->names[ds->key];
    uint64_t n = std::min<uint64_t>(max_rows, (uint64_t)ds->key_len[ds->key] - ds->next);      // a batch never spans two contigs
    if (!name.empty()) n = std::min<uint64_t>(n, std::max<uint64_t>(1, (uint64_t)INT32_MAX / name.size()));   // Utf8 offsets are int32
    n = std::min<uint64_t>(n, (uint64_t)INT32_MAX);
    // zero_based: positions [0, len); else [1, len + 1), never adding slot 0 (coverage.rs:294-301)
    const uint64_t first = (ds->zero_based ? 0u : 1u) + ds->next;
    std::vector<int32_t> p32(n); std::vector<int16_t> c16(n);
    const ivx_status st = ivx_depth_profile_expand(s->ctx, ds->profile, IVX_MEM_HOST, ds->key, (uint32_t)first, n, ds->zero_based ? 0 : 1,
                                                   p32.data(), c16.data());
    if (st != IVX_OK) return fail_ivx(s, st);
    const std::vector<uint32_t> ids(n, ds->key);
    make_utf8(contig, ds->names, ids.data(), (int64_t)n); make_schema(contig_schema, "u", "contig", true);
    make_primitive<int32_t>(pos, p32.data(), (int64_t)n, nullptr); make_schema(pos_schema, "i", "pos", false);
    make_primitive<int16_t>(coverage, c16.data(), (int64_t)n, nullptr); make_schema(coverage_schema, "s", "coverage", false);
    ds->next += n;
    return 0;
}

extern "C" void brh_depth_per_base_close(brh_depth_stream *ds)
{
    if (!ds) return;
    if (ds->profile) ivx_depth_profile_free(ds->profile);
    delete ds;
}

// ---- streaming depth(): the reference's accumulate_partition (physical_exec.rs:269-329) as a push interface -- one depth
// profile per pushed batch, kept on a stack that is merged like a binary counter, and merge_*_results (:367-463) at finish
struct brh_depth_push {
    brh_session *s = nullptr;
    bool dense = false, finished = false;
    uint32_t filter_flag = 0, min_mapq = 0;
    std::vector<std::string> names;                     // key id -> contig: byte order (dense), arrival order (sparse)
    std::unordered_map<std::string, uint32_t> ids;
    std::vector<uint32_t> key_len;                      // dense only
    std::vector<ivx_index *> stack;                     // profiles not yet merged, the oldest first
    uint32_t built_nk = 0;                              // the most keys a profile of the stack was built with
    uint32_t nk() const { return (uint32_t)std::max<size_t>(names.size(), 1); }
};

namespace {

int depth_push_check(brh_depth_push *dp)
{
    return dp->finished ? fail(dp->s, "depth stream: already finished") : 0;
}

// the two profiles on top of the stack -> their sum
int depth_push_merge_top(brh_depth_push *dp)
{
    ivx_index *a = dp->stack[dp->stack.size() - 2], *b = dp->stack.back(), *m = nullptr;
    const ivx_status st = ivx_depth_profile_merge(dp->s->ctx, a, b, &m);
    if (st != IVX_OK) return fail_ivx(dp->s, st);
    ivx_depth_profile_free(a); ivx_depth_profile_free(b);
    dp->stack.pop_back();
    dp->stack.back() = m;
    return 0;
}

// everything pushed so far as ONE profile on the stack (an empty one when nothing was)
int depth_push_merge_all(brh_depth_push *dp)
{
    while (dp->stack.size() > 1) if (depth_push_merge_top(dp)) return 1;
    if (dp->stack.empty()) {
        ivx_index *e = nullptr;
        const ivx_status st = ivx_depth_profile_build(dp->s->ctx, IVX_MEM_HOST, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                                                      nullptr, nullptr, nullptr, nullptr, 0, dp->nk(), dp->dense ? dp->key_len.data() : nullptr,
                                                      dp->filter_flag, dp->min_mapq, &e);
        if (st != IVX_OK) return fail_ivx(dp->s, st);
        dp->stack.push_back(e);
        dp->built_nk = std::max(dp->built_nk, dp->nk());
    }
    return 0;
}

int ProfileSource::open(brh_depth_push *p)
{
    if (depth_push_check(p) || depth_push_merge_all(p)) return 1;
    dp = p; profile = p->stack[0]; nk = p->built_nk; known = std::min<uint32_t>((uint32_t)p->names.size(), p->built_nk);
    names = &p->names; key_len = p->dense ? &p->key_len : nullptr; by_name = !p->dense;
    return 0;
}

uint32_t ProfileSource::id_of(std::string_view name) const
{
    if (!dp) return in.dict.id_of(name);
    auto it = dp->ids.find(std::string(name));
    return it == dp->ids.end() ? IVX_NULL_IDX : it->second;
}

}  // namespace

// the rows [lo[k], lo[k + 1]) of every key k, the keys taken in byte order of their names: for each output row the input row it
// comes from.  (Rows are grouped by key ascending, so a key's rows are contiguous.)  Not part of the C interface; it has external
// linkage so that a stand-alone program can link it and check it on the CPU.
void brh_depth_rows_in_name_order(const std::vector<std::string> &names, const uint32_t *key, uint64_t n, std::vector<uint64_t> *src)
{
    std::vector<uint64_t> lo(names.size() + 1, n);
    for (uint64_t i = n; i-- > 0;) if (key[i] < names.size()) lo[key[i]] = i;
    for (size_t k = names.size(); k-- > 0;) if (lo[k] > lo[k + 1]) lo[k] = lo[k + 1];       // a key without rows starts where the next one does
    std::vector<uint32_t> order(names.size());
    for (uint32_t k = 0; k < names.size(); k++) order[k] = k;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return names[a] < names[b]; });
    src->clear(); src->reserve(n);
    for (uint32_t k : order) for (uint64_t i = lo[k]; i < lo[k + 1]; i++) src->push_back(i);
}

extern "C" int brh_depth_push_open(brh_session *s, brh_batch lengths, uint32_t filter_flag, uint32_t min_mapq, brh_depth_push **out)
{
    if (!s) return 1;
    if (!out) return fail(s, "depth stream: null out");
    *out = nullptr;
    std::unique_ptr<brh_depth_push> dp(new brh_depth_push());
    dp->s = s; dp->filter_flag = filter_flag; dp->min_mapq = min_mapq;
    dp->dense = lengths.array != nullptr;
    if (dp->dense) {
        NameDict dict;
        if (load_lengths(s, lengths, &dict, &dp->key_len)) return 1;
        dp->names = dict.names;
        for (uint32_t i = 0; i < dp->names.size(); i++) dp->ids.emplace(dp->names[i], i);
    }
    *out = dp.release();
    return 0;
}

extern "C" int brh_depth_push_batch(brh_depth_push *dp, brh_batch reads)
{
    if (!dp) return 1;
    brh_session *s = dp->s;
    if (depth_push_check(dp)) return 1;
    if (reads.array && reads.schema && reads.array->length == 0) return 0;             // physical_exec.rs:282-284
    DepthInputs in;
    if (in.load(s, reads, brh_batch{nullptr, nullptr}, brh_batch{nullptr, nullptr})) return 1;
    // the batch's own ids (byte order of ITS names) -> the stream's
    std::vector<uint32_t> to_stream(in.dict.names.size());
    for (size_t i = 0; i < to_stream.size(); i++) {
        auto it = dp->ids.find(in.dict.names[i]);
        if (it != dp->ids.end()) to_stream[i] = it->second;
        else if (dp->dense) to_stream[i] = IVX_NULL_IDX;                                 // events.rs:247-260
        else {
            to_stream[i] = (uint32_t)dp->names.size();
            dp->ids.emplace(in.dict.names[i], to_stream[i]);
            dp->names.push_back(in.dict.names[i]);
        }
    }
    for (uint32_t &k : in.rkey) if (k != IVX_NULL_IDX) k = to_stream[k];
    ivx_index *p = nullptr;
    const ivx_status st = in.profile(s->ctx, DepthInputs::of_stream(dp->nk(), dp->dense ? dp->key_len.data() : nullptr), dp->filter_flag, dp->min_mapq, &p);
    if (st != IVX_OK) return fail_ivx(s, st);
    dp->stack.push_back(p);
    dp->built_nk = std::max(dp->built_nk, dp->nk());
    // a binary counter: merge while the new top has at least half the steps of the profile below it
    while (dp->stack.size() > 1 &&
           2 * ivx_depth_profile_steps(dp->stack.back()) >= ivx_depth_profile_steps(dp->stack[dp->stack.size() - 2]))
        if (depth_push_merge_top(dp)) return 1;
    return 0;
}

extern "C" int brh_depth_push_finish(brh_depth_push *dp,
                                     ArrowArray *contig, ArrowSchema *contig_schema, ArrowArray *pos_start, ArrowSchema *pos_start_schema,
                                     ArrowArray *pos_end, ArrowSchema *pos_end_schema, ArrowArray *coverage, ArrowSchema *coverage_schema)
{
    if (!dp) return 1;
    brh_session *s = dp->s;
    if (depth_push_check(dp) || depth_push_merge_all(dp)) return 1;
    const ivx_index *p = dp->stack[0];
    uint64_t m = 0, m2 = 0;
    ivx_status st = ivx_depth_profile_blocks(s->ctx, p, IVX_MEM_HOST, nullptr, nullptr, nullptr, nullptr, 0, &m);
    if (st != IVX_OK) return fail_ivx(s, st);
    std::vector<uint32_t> ok(m ? m : 1), os(m ? m : 1), oe(m ? m : 1); std::vector<int32_t> oc(m ? m : 1);
    if (m) {
        st = ivx_depth_profile_blocks(s->ctx, p, IVX_MEM_HOST, ok.data(), os.data(), oe.data(), oc.data(), m, &m2);
        if (st != IVX_OK) return fail_ivx(s, st);
    }
    ivx_depth_profile_free(dp->stack[0]);
    dp->stack.clear();
    dp->finished = true;
    // ---- sparse: the stream's ids are in arrival order, the output is in byte order of the names (coverage.rs:75-76)
    std::vector<uint64_t> src;
    if (!dp->dense) brh_depth_rows_in_name_order(dp->names, ok.data(), m2, &src);
    // ---- schema.rs:28-41: contig Utf8, pos_start / pos_end Int32 (`as i32`), coverage Int16 (`as i16`)
    std::vector<uint32_t> oid(m2 ? m2 : 1);
    std::vector<int32_t> o32s(m2 ? m2 : 1), o32e(m2 ? m2 : 1); std::vector<int16_t> o16(m2 ? m2 : 1);
    for (uint64_t i = 0; i < m2; i++) {
        const uint64_t j = dp->dense ? i : src[i];
        oid[i] = ok[j]; o32s[i] = (int32_t)os[j]; o32e[i] = (int32_t)oe[j]; o16[i] = (int16_t)oc[j];
    }
    make_utf8(contig, dp->names, oid.data(), (int64_t)m2); make_schema(contig_schema, "u", "contig", true);
    make_primitive<int32_t>(pos_start, o32s.data(), (int64_t)m2, nullptr); make_schema(pos_start_schema, "i", "pos_start", false);
    make_primitive<int32_t>(pos_end, o32e.data(), (int64_t)m2, nullptr); make_schema(pos_end_schema, "i", "pos_end", false);
    make_primitive<int16_t>(coverage, o16.data(), (int64_t)m2, nullptr); make_schema(coverage_schema, "s", "coverage", false);
    return 0;
}

extern "C" int brh_depth_push_finish_per_base(brh_depth_push *dp, int zero_based, brh_depth_stream **out)
{
    if (!dp) return 1;
    brh_session *s = dp->s;
    if (!out) return fail(s, "depth stream: null out");
    *out = nullptr;
    if (depth_push_check(dp)) return 1;
    if (!dp->dense)                         // physical_exec.rs:299-303
        return fail(s, "per_base mode requires dense accumulation (BAM header with contig lengths). "
                       "Sparse fallback (e.g. MemTable) is not supported for per_base output.");
    if (depth_push_merge_all(dp)) return 1;
    std::unique_ptr<brh_depth_stream> ds(new brh_depth_stream());
    ds->s = s; ds->zero_based = zero_based != 0;
    ds->names = dp->names; ds->key_len = dp->key_len;
    ds->seen.assign(dp->nk(), 0);
    uint64_t steps = 0;
    const ivx_status st = ivx_depth_profile_read(s->ctx, dp->stack[0], IVX_MEM_HOST, nullptr, nullptr, nullptr, ds->seen.data(), 0, &steps);
    if (st != IVX_OK) return fail_ivx(s, st);
    if (ds->names.empty()) ds->seen.assign(ds->seen.size(), 0);     // (an empty length table: key 0 stands for no contig)
    ds->profile = dp->stack[0];                                     // the profile moves into the pull stream
    dp->stack.clear();
    dp->finished = true;
    *out = ds.release();
    return 0;
}

extern "C" void brh_depth_push_close(brh_depth_push *dp)
{
    if (!dp) return;
    for (ivx_index *p : dp->stack) ivx_depth_profile_free(p);
    delete dp;
}

// ---- depth region summaries (ivx_depth_profile_summarize): bases, coverage sum and bases at or above each threshold per row
// of a regions table -- mean depth per target, bases at 10x / 20x / 30x (samtools bedcov, mosdepth --by / --thresholds)
namespace {

// one coordinate column as int64, a UInt64 beyond that saturated (every value is clamped to [0, 2^32-1] afterwards anyway)
int region_coords(brh_session *s, const PosCol &p, std::vector<int64_t> *out)
{
    if (null_count(p.a) > 0) return fail(s, "coordinate column contains null values; requires non-null coordinates");
    const int64_t n = p.a->length, o = p.a->offset;
    out->resize((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        switch (p.fmt) {
        case 'i': (*out)[i] = ((const int32_t *)p.a->buffers[1])[o + i]; break;
        case 'l': (*out)[i] = ((const int64_t *)p.a->buffers[1])[o + i]; break;
        case 'I': (*out)[i] = ((const uint32_t *)p.a->buffers[1])[o + i]; break;
        default: { const uint64_t v = ((const uint64_t *)p.a->buffers[1])[o + i]; (*out)[i] = v > (uint64_t)INT64_MAX ? INT64_MAX : (int64_t)v; }
        }
    }
    return 0;
}

// The rows of a regions table as the closed u32 regions the profile calls take.  The keys are the ids the profile source gives
// (IVX_NULL_IDX, or an id of src.known or more: a contig the profile does not know, coverage 0 everywhere: `unknown`, answered by
// the caller).  A region that is empty whatever the coverage gets the skip mark.  key_len (null: no length table) gives the
// domain the per-base rows have: [0, len - 1] when zero_based, else [1, len] without the step at position 0.
struct RegionRows {
    uint64_t n = 0;
    std::vector<uint32_t> qk, qs, qe, key_hi;
    std::vector<uint8_t> unknown;
    uint32_t pos_lo = 0;
    bool has_len = false, skip_pos0 = false;

    int load(brh_session *s, const char *what, const ProfileSource &src, int zero_based, brh_batch regions, brh_columns cols, int end_exclusive)
    {
        const uint32_t n_keys = src.known;
        const std::vector<uint32_t> *key_len = src.key_len;
        if (!regions.array || !regions.schema) return fail(s, std::string(what) + ": null regions batch");
        if (cols.n_keys != 1 || !cols.keys || !cols.start || !cols.end)
            return fail(s, std::string(what) + ": the regions take one contig, one start and one end column");
        StrCol contig; PosCol ps, pe;
        std::vector<int64_t> s64, e64;
        if (get_contig(s, regions, cols.keys[0], &contig) || get_pos(s, regions, cols.start, "start", &ps) || get_pos(s, regions, cols.end, "end", &pe) ||
            region_coords(s, ps, &s64) || region_coords(s, pe, &e64)) return 1;
        n = (uint64_t)regions.array->length;
        qk.assign(n ? n : 1, 0); qs.assign(n ? n : 1, 0); qe.assign(n ? n : 1, 0);
        unknown.assign(n ? n : 1, 0);
        has_len = key_len != nullptr;
        pos_lo = (key_len && !zero_based) ? 1u : 0u;
        skip_pos0 = key_len && !zero_based;
        if (key_len) {
            key_hi.assign(std::max<size_t>(key_len->size(), n_keys), 0);
            for (size_t k = 0; k < key_len->size(); k++) key_hi[k] = zero_based ? ((*key_len)[k] ? (*key_len)[k] - 1u : 0u) : (*key_len)[k];
        }
        std::string_view last; uint32_t last_id = IVX_NULL_IDX; bool have = false;
        for (uint64_t i = 0; i < n; i++) {
            int64_t a = s64[i], b = e64[i];
            bool empty = false;
            if (end_exclusive) { if (b <= a) empty = true; else b -= 1; }
            a = std::min<int64_t>(std::max<int64_t>(a, 0), (int64_t)UINT32_MAX);
            b = std::min<int64_t>(std::max<int64_t>(b, 0), (int64_t)UINT32_MAX);
            qs[i] = (uint32_t)a; qe[i] = (uint32_t)b;
            uint32_t k = IVX_NULL_IDX;
            if (!contig.null_at((int64_t)i)) {
                const std::string_view name = contig.at((int64_t)i);
                if (!have || name != last) { last_id = src.id_of(name); last = name; have = true; }
                k = last_id;
            }
            if (k >= n_keys) { unknown[i] = !empty && b >= a; k = IVX_NULL_IDX; }
            else if (empty || (key_len && zero_based && (*key_len)[k] == 0)) k = IVX_NULL_IDX;        // (a contig of length 0 has no position)
            qk[i] = k;
        }
        return 0;
    }
    const uint32_t *hi() const { return has_len ? key_hi.data() : nullptr; }
};

// The regions of `regions` summarised over `profile` (RegionRows for the keys, the domain and the unknown contigs)
int summarize_regions(brh_session *s, const ProfileSource &src, int zero_based, brh_batch regions, brh_columns cols, int end_exclusive,
                      const int32_t *thresholds, uint32_t n_thr,
                      ArrowArray *bases, ArrowSchema *bases_schema, ArrowArray *sum, ArrowSchema *sum_schema, ArrowArray *ge, ArrowSchema *ge_schemas)
{
    if (!regions.array || !regions.schema) return fail(s, "depth_regions: null regions batch");
    if (cols.n_keys != 1 || !cols.keys || !cols.start || !cols.end) return fail(s, "depth_regions: the regions take one contig, one start and one end column");
    if (n_thr > IVX_DEPTH_MAX_THRESHOLDS) return fail(s, "depth_regions: more than 8 thresholds");
    if (n_thr && (!thresholds || !ge || !ge_schemas)) return fail(s, "depth_regions: null thresholds or threshold outputs");
    RegionRows r;
    if (r.load(s, "depth_regions", src, zero_based, regions, cols, end_exclusive)) return 1;
    const uint64_t n = r.n;
    std::vector<int64_t> ol(n ? n : 1, 0), os(n ? n : 1, 0), og((size_t)n_thr * n + 1, 0);
    const ivx_status st = ivx_depth_profile_summarize(s->ctx, src.profile, IVX_MEM_HOST, r.qk.data(), r.qs.data(), r.qe.data(), n, r.pos_lo,
                                                      r.hi(), r.skip_pos0, thresholds, n_thr,
                                                      ol.data(), os.data(), n_thr ? og.data() : nullptr);
    if (st != IVX_OK) return fail_ivx(s, st);
    for (uint64_t i = 0; i < n; i++) {
        if (!r.unknown[i]) continue;
        ol[i] = (int64_t)r.qe[i] - (int64_t)r.qs[i] + 1;
        for (uint32_t j = 0; j < n_thr; j++) og[(size_t)j * n + i] = thresholds[j] <= 0 ? ol[i] : 0;
    }
    make_primitive<int64_t>(bases, ol.data(), (int64_t)n, nullptr); make_schema(bases_schema, "l", "bases", false);
    make_primitive<int64_t>(sum, os.data(), (int64_t)n, nullptr); make_schema(sum_schema, "l", "sum", false);
    for (uint32_t j = 0; j < n_thr; j++) {
        make_primitive<int64_t>(&ge[j], og.data() + (size_t)j * n, (int64_t)n, nullptr);
        make_schema(&ge_schemas[j], "l", ("bases_ge_" + std::to_string(thresholds[j])).c_str(), false);
    }
    return 0;
}

// The same rows ranked over `profile` (ivx_depth_profile_quantiles): bases, and min / max / the quantiles, NULL where bases = 0
int rank_regions(brh_session *s, const ProfileSource &src, int zero_based, brh_batch regions, brh_columns cols, int end_exclusive,
                 const uint32_t *q_num, uint32_t n_q, uint32_t q_den,
                 ArrowArray *bases, ArrowSchema *bases_schema, ArrowArray *mn, ArrowSchema *mn_schema, ArrowArray *mx, ArrowSchema *mx_schema,
                 ArrowArray *q, ArrowSchema *q_schemas)
{
    if (n_q > IVX_DEPTH_MAX_QUANTILES) return fail(s, "depth_region_quantiles: more than 8 quantiles");
    if (n_q && (!q_num || !q || !q_schemas)) return fail(s, "depth_region_quantiles: null q_num or quantile outputs");
    RegionRows r;
    if (r.load(s, "depth_region_quantiles", src, zero_based, regions, cols, end_exclusive)) return 1;
    const uint64_t n = r.n;
    std::vector<int64_t> ol(n ? n : 1, 0);
    std::vector<int32_t> omn(n ? n : 1, 0), omx(n ? n : 1, 0), oq((size_t)n_q * n + 1, 0);
    const ivx_status st = ivx_depth_profile_quantiles(s->ctx, src.profile, IVX_MEM_HOST, r.qk.data(), r.qs.data(), r.qe.data(), n, r.pos_lo,
                                                      r.hi(), r.skip_pos0, q_num, n_q, q_den,
                                                      ol.data(), omn.data(), omx.data(), n_q ? oq.data() : nullptr);
    if (st != IVX_OK) return fail_ivx(s, st);
    std::vector<uint8_t> valid(n ? n : 1, 0);
    for (uint64_t i = 0; i < n; i++) {
        if (r.unknown[i]) ol[i] = (int64_t)r.qe[i] - (int64_t)r.qs[i] + 1;      // (coverage 0 everywhere: the zeros are in place)
        valid[i] = ol[i] > 0;
    }
    make_primitive<int64_t>(bases, ol.data(), (int64_t)n, nullptr); make_schema(bases_schema, "l", "bases", false);
    make_primitive<int32_t>(mn, omn.data(), (int64_t)n, valid.data()); make_schema(mn_schema, "i", "min", true);
    make_primitive<int32_t>(mx, omx.data(), (int64_t)n, valid.data()); make_schema(mx_schema, "i", "max", true);
    for (uint32_t j = 0; j < n_q; j++) {
        make_primitive<int32_t>(&q[j], oq.data() + (size_t)j * n, (int64_t)n, valid.data());
        make_schema(&q_schemas[j], "i", ("q_" + std::to_string(q_num[j]) + "_" + std::to_string(q_den)).c_str(), true);
    }
    return 0;
}

}  // namespace

extern "C" int brh_depth_regions(brh_session *s, brh_batch reads, brh_batch prior, brh_batch lengths, brh_batch regions, brh_columns region_cols,
                                 int zero_based, int end_exclusive, uint32_t filter_flag, uint32_t min_mapq,
                                 const int32_t *thresholds, uint32_t n_thr,
                                 ArrowArray *bases, ArrowSchema *bases_schema, ArrowArray *sum, ArrowSchema *sum_schema,
                                 ArrowArray *ge, ArrowSchema *ge_schemas)
{
    if (!s) return 1;
    ProfileSource src;
    if (src.open(s, reads, prior, lengths, filter_flag, min_mapq)) return 1;
    return summarize_regions(s, src, zero_based, regions, region_cols, end_exclusive, thresholds, n_thr, bases, bases_schema, sum, sum_schema, ge, ge_schemas);
}

extern "C" int brh_depth_push_regions(brh_depth_push *dp, brh_batch regions, brh_columns region_cols, int zero_based, int end_exclusive,
                                      const int32_t *thresholds, uint32_t n_thr,
                                      ArrowArray *bases, ArrowSchema *bases_schema, ArrowArray *sum, ArrowSchema *sum_schema,
                                      ArrowArray *ge, ArrowSchema *ge_schemas)
{
    if (!dp) return 1;
    ProfileSource src;
    if (src.open(dp)) return 1;
    return summarize_regions(dp->s, src, zero_based, regions, region_cols, end_exclusive, thresholds, n_thr, bases, bases_schema, sum, sum_schema, ge, ge_schemas);
}

extern "C" int brh_depth_region_quantiles(brh_session *s, brh_batch reads, brh_batch prior, brh_batch lengths, brh_batch regions, brh_columns region_cols,
                                          int zero_based, int end_exclusive, uint32_t filter_flag, uint32_t min_mapq,
                                          const uint32_t *q_num, uint32_t n_q, uint32_t q_den,
                                          ArrowArray *bases, ArrowSchema *bases_schema, ArrowArray *mn, ArrowSchema *mn_schema,
                                          ArrowArray *mx, ArrowSchema *mx_schema, ArrowArray *q, ArrowSchema *q_schemas)
{
    if (!s) return 1;
    ProfileSource src;
    if (src.open(s, reads, prior, lengths, filter_flag, min_mapq)) return 1;
    return rank_regions(s, src, zero_based, regions, region_cols, end_exclusive, q_num, n_q, q_den, bases, bases_schema, mn, mn_schema, mx, mx_schema, q, q_schemas);
}

extern "C" int brh_depth_push_region_quantiles(brh_depth_push *dp, brh_batch regions, brh_columns region_cols, int zero_based, int end_exclusive,
                                               const uint32_t *q_num, uint32_t n_q, uint32_t q_den,
                                               ArrowArray *bases, ArrowSchema *bases_schema, ArrowArray *mn, ArrowSchema *mn_schema,
                                               ArrowArray *mx, ArrowSchema *mx_schema, ArrowArray *q, ArrowSchema *q_schemas)
{
    if (!dp) return 1;
    ProfileSource src;
    if (src.open(dp)) return 1;
    return rank_regions(dp->s, src, zero_based, regions, region_cols, end_exclusive, q_num, n_q, q_den, bases, bases_schema, mn, mn_schema, mx, mx_schema, q, q_schemas);
}

// ---- depth coverage classes (ivx_depth_profile_quantize / ivx_depth_profile_hist): the maximal intervals of one coverage bin,
// and the bases per coverage value of every contig (mosdepth --quantize / dist, bedtools genomecov)
namespace {

// The domain of every key of a profile of nk keys, as RegionRows has it for the regions: key_len (null: no length table) gives
// [0, len - 1] when zero_based, else [1, len] without the step at position 0.  `drop` marks the keys that never go out: the
// ones the dictionary does not name (key 0 of an empty dictionary) and, zero_based, a contig of length 0, which has no position.
struct ClassDomain {
    std::vector<uint32_t> key_hi;
    std::vector<uint8_t> drop;
    uint32_t pos_lo = 0;
    bool has_len = false, skip_pos0 = false;
    ClassDomain(const ProfileSource &src, int zero_based)
    {
        const uint32_t nk = src.nk, known = src.known;
        const std::vector<uint32_t> *key_len = src.key_len;
        has_len = key_len != nullptr;
        pos_lo = (key_len && !zero_based) ? 1u : 0u;
        skip_pos0 = key_len && !zero_based;
        drop.assign(nk, 0);
        for (uint32_t k = known; k < nk; k++) drop[k] = 1;
        if (!key_len) return;
        key_hi.assign(std::max<size_t>(key_len->size(), nk), 0);
        for (size_t k = 0; k < key_len->size(); k++) {
            const uint32_t len = (*key_len)[k];
            key_hi[k] = zero_based ? (len ? len - 1u : 0u) : len;
            if (zero_based && !len && k < nk) drop[k] = 1;
        }
    }
    const uint32_t *hi() const { return has_len ? key_hi.data() : nullptr; }
};

// the keys < known in the order their rows go out: ascending ids, or (by_name) the byte order of their names
std::vector<uint32_t> class_key_order(const ProfileSource &src)
{
    std::vector<uint32_t> order(src.known);
    for (uint32_t k = 0; k < src.known; k++) order[k] = k;
    if (src.by_name) std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return (*src.names)[a] < (*src.names)[b]; });
    return order;
}

int quantize_profile(brh_session *s, const ProfileSource &src, int zero_based, int end_exclusive, int touched_only,
                     const int32_t *cuts, uint32_t n_cuts, uint32_t emit_mask,
                     ArrowArray *contig, ArrowSchema *contig_schema, ArrowArray *start, ArrowSchema *start_schema,
                     ArrowArray *end, ArrowSchema *end_schema, ArrowArray *bin, ArrowSchema *bin_schema)
{
    const ClassDomain d(src, zero_based);
    const uint32_t nk = src.nk;
    auto call = [&](uint32_t *ok, uint32_t *os, uint32_t *oe, uint32_t *oc, uint64_t cap, uint64_t *m) {
        return ivx_depth_profile_quantize(s->ctx, src.profile, IVX_MEM_HOST, d.pos_lo, d.hi(), d.skip_pos0, touched_only != 0, cuts, n_cuts, emit_mask,
                                          ok, os, oe, oc, cap, m);
    };
    uint64_t m = 0, m2 = 0;
    ivx_status st = call(nullptr, nullptr, nullptr, nullptr, 0, &m);
    if (st != IVX_OK) return fail_ivx(s, st);
    std::vector<uint32_t> ok(m ? m : 1), os(m ? m : 1), oe(m ? m : 1), oc(m ? m : 1);
    if (m) {
        st = call(ok.data(), os.data(), oe.data(), oc.data(), m, &m2);
        if (st != IVX_OK) return fail_ivx(s, st);
    }
    // the rows are grouped by key ascending: [lo[k], lo[k + 1]) are key k's
    std::vector<uint64_t> lo((size_t)nk + 1, m2);
    for (uint64_t i = m2; i-- > 0;) if (ok[i] < nk) lo[ok[i]] = i;
    for (size_t k = nk; k-- > 0;) if (lo[k] > lo[k + 1]) lo[k] = lo[k + 1];
    std::vector<uint32_t> oid; std::vector<int64_t> o64s, o64e; std::vector<int32_t> obin;
    for (uint32_t k : class_key_order(src)) {
        if (d.drop[k]) continue;
        for (uint64_t i = lo[k]; i < lo[k + 1]; i++) {
            oid.push_back(k); o64s.push_back((int64_t)os[i]); o64e.push_back((int64_t)oe[i] + (end_exclusive ? 1 : 0)); obin.push_back((int32_t)oc[i]);
        }
    }
    const int64_t n = (int64_t)oid.size();
    if (!n) { oid.push_back(0); o64s.push_back(0); o64e.push_back(0); obin.push_back(0); }
    make_utf8(contig, *src.names, oid.data(), n); make_schema(contig_schema, "u", "contig", true);
    make_primitive<int64_t>(start, o64s.data(), n, nullptr); make_schema(start_schema, "l", "start", false);
    make_primitive<int64_t>(end, o64e.data(), n, nullptr); make_schema(end_schema, "l", "end", false);
    make_primitive<int32_t>(bin, obin.data(), n, nullptr); make_schema(bin_schema, "i", "bin", false);
    return 0;
}

int dist_profile(brh_session *s, const ProfileSource &src, int zero_based, int touched_only, int32_t v_lo, uint32_t n_bins,
                 ArrowArray *contig, ArrowSchema *contig_schema, ArrowArray *coverage, ArrowSchema *coverage_schema,
                 ArrowArray *bases, ArrowSchema *bases_schema)
{
    if (n_bins == 0 || n_bins > IVX_DEPTH_MAX_BINS) return fail(s, "depth_dist: n_bins outside 1 .. 65536");
    const ClassDomain d(src, zero_based);
    std::vector<int64_t> h((size_t)src.nk * n_bins, 0);
    const ivx_status st = ivx_depth_profile_hist(s->ctx, src.profile, IVX_MEM_HOST, d.pos_lo, d.hi(), d.skip_pos0, touched_only != 0, v_lo, n_bins, h.data());
    if (st != IVX_OK) return fail_ivx(s, st);
    std::vector<uint32_t> oid; std::vector<int32_t> ocov; std::vector<int64_t> obases;
    for (uint32_t k : class_key_order(src)) {
        if (d.drop[k]) continue;
        for (uint32_t b = 0; b < n_bins; b++) {
            const int64_t c = h[(size_t)k * n_bins + b];
            if (c <= 0) continue;
            oid.push_back(k); ocov.push_back((int32_t)std::min<int64_t>((int64_t)v_lo + b, INT32_MAX)); obases.push_back(c);
        }
    }
    const int64_t n = (int64_t)oid.size();
    if (!n) { oid.push_back(0); ocov.push_back(0); obases.push_back(0); }
    make_utf8(contig, *src.names, oid.data(), n); make_schema(contig_schema, "u", "contig", true);
    make_primitive<int32_t>(coverage, ocov.data(), n, nullptr); make_schema(coverage_schema, "i", "coverage", false);
    make_primitive<int64_t>(bases, obases.data(), n, nullptr); make_schema(bases_schema, "l", "bases", false);
    return 0;
}

}  // namespace

extern "C" int brh_depth_quantize(brh_session *s, brh_batch reads, brh_batch prior, brh_batch lengths, int zero_based, int end_exclusive,
                                  int touched_only, uint32_t filter_flag, uint32_t min_mapq,
                                  const int32_t *cuts, uint32_t n_cuts, uint32_t emit_mask,
                                  ArrowArray *contig, ArrowSchema *contig_schema, ArrowArray *start, ArrowSchema *start_schema,
                                  ArrowArray *end, ArrowSchema *end_schema, ArrowArray *bin, ArrowSchema *bin_schema)
{
    if (!s) return 1;
    ProfileSource src;
    if (src.open(s, reads, prior, lengths, filter_flag, min_mapq)) return 1;
    return quantize_profile(s, src, zero_based, end_exclusive, touched_only, cuts, n_cuts, emit_mask,
                            contig, contig_schema, start, start_schema, end, end_schema, bin, bin_schema);
}

extern "C" int brh_depth_push_quantize(brh_depth_push *dp, int zero_based, int end_exclusive, int touched_only,
                                       const int32_t *cuts, uint32_t n_cuts, uint32_t emit_mask,
                                       ArrowArray *contig, ArrowSchema *contig_schema, ArrowArray *start, ArrowSchema *start_schema,
                                       ArrowArray *end, ArrowSchema *end_schema, ArrowArray *bin, ArrowSchema *bin_schema)
{
    if (!dp) return 1;
    ProfileSource src;
    if (src.open(dp)) return 1;
    return quantize_profile(dp->s, src, zero_based, end_exclusive, touched_only, cuts, n_cuts, emit_mask,
                            contig, contig_schema, start, start_schema, end, end_schema, bin, bin_schema);
}

extern "C" int brh_depth_dist(brh_session *s, brh_batch reads, brh_batch prior, brh_batch lengths, int zero_based, int touched_only,
                              uint32_t filter_flag, uint32_t min_mapq, int32_t v_lo, uint32_t n_bins,
                              ArrowArray *contig, ArrowSchema *contig_schema, ArrowArray *coverage, ArrowSchema *coverage_schema,
                              ArrowArray *bases, ArrowSchema *bases_schema)
{
    if (!s) return 1;
    ProfileSource src;
    if (src.open(s, reads, prior, lengths, filter_flag, min_mapq)) return 1;
    return dist_profile(s, src, zero_based, touched_only, v_lo, n_bins, contig, contig_schema, coverage, coverage_schema, bases, bases_schema);
}

extern "C" int brh_depth_push_dist(brh_depth_push *dp, int zero_based, int touched_only, int32_t v_lo, uint32_t n_bins,
                                   ArrowArray *contig, ArrowSchema *contig_schema, ArrowArray *coverage, ArrowSchema *coverage_schema,
                                   ArrowArray *bases, ArrowSchema *bases_schema)
{
    if (!dp) return 1;
    ProfileSource src;
    if (src.open(dp)) return 1;
    return dist_profile(dp->s, src, zero_based, touched_only, v_lo, n_bins, contig, contig_schema, coverage, coverage_schema, bases, bases_schema);
}

// ---- f3: payload gather
namespace {

// bytes per element of a fixed-width Arrow format string, 0 if it is not one we gather
uint32_t fixed_width(const char *f)
{
    if (std::strlen(f) == 1) {
        switch (f[0]) {
        case 'c': case 'C': return 1;
        case 's': case 'S': case 'e': return 2;
        case 'i': case 'I': case 'f': return 4;
        case 'l': case 'L': case 'g': return 8;
        default: return 0;
        }
    }
    if (!std::strncmp(f, "tdD", 3) || !std::strncmp(f, "tts", 3) || !std::strncmp(f, "ttm", 3)) return 4;      // date32, time32
    if (!std::strncmp(f, "tdm", 3) || !std::strncmp(f, "ttu", 3) || !std::strncmp(f, "ttn", 3)) return 8;      // date64, time64
    if (!std::strncmp(f, "ts", 2) || !std::strncmp(f, "tD", 2)) return 8;                                       // timestamp, duration
    if (!std::strncmp(f, "d:", 2)) {                                                                            // decimal128 / decimal256
        int commas = 0; const char *last = nullptr;
        for (const char *q = f; *q; q++) if (*q == ',') { commas++; last = q; }
        if (commas < 2) return 16;
        const int bits = std::atoi(last + 1);
        return bits == 128 ? 16 : bits == 256 ? 32 : 0;
    }
    if (!std::strncmp(f, "w:", 2)) { const int w = std::atoi(f + 2); return (w == 1 || w == 2 || w == 4 || w == 8 || w == 16 || w == 32) ? (uint32_t)w : 0; }
    return 0;
}

// validity bitmap of `a` re-based to bit 0 (nullptr when there are no nulls)
const uint8_t *rebased_validity(const ArrowArray *a, std::vector<uint8_t> *store)
{
    if (a->n_buffers < 1 || !a->buffers[0] || null_count(a) == 0) return nullptr;
    const uint8_t *v = (const uint8_t *)a->buffers[0];
    if (a->offset % 8 == 0) return v + a->offset / 8;
    store->assign((size_t)(a->length + 7) / 8, 0);
    for (int64_t i = 0; i < a->length; i++) { const int64_t j = i + a->offset; if ((v[j >> 3] >> (j & 7)) & 1) (*store)[i >> 3] |= (uint8_t)(1u << (i & 7)); }
    return store->data();
}

// an owned copy (offset 0) of a flat array: fixed-width primitives, Boolean, Utf8 / LargeUtf8 / Binary / LargeBinary --
// the value types a dictionary-encoded payload column keeps its values in; false for anything else
bool copy_flat_array(const ArrowArray *src, const char *f, ArrowArray *dst)
{
    std::memset(dst, 0, sizeof *dst);
    const int64_t n = src->length, o = src->offset;
    OutPriv *p = new OutPriv();
    int nb = 2;
    const bool s32 = !std::strcmp(f, "u") || !std::strcmp(f, "z"), s64 = !std::strcmp(f, "U") || !std::strcmp(f, "Z");
    if (s32 || s64) {
        const size_t ow = s64 ? 8 : 4;
        const uint8_t *off = (const uint8_t *)src->buffers[1] + (size_t)o * ow;
        const int64_t base = s64 ? ((const int64_t *)off)[0] : (int64_t)((const int32_t *)off)[0];
        const int64_t end = s64 ? ((const int64_t *)off)[n] : (int64_t)((const int32_t *)off)[n];
        void *oo = std::malloc((size_t)(n + 1) * ow);
        for (int64_t i = 0; i <= n; i++) {
            if (s64) ((int64_t *)oo)[i] = ((const int64_t *)off)[i] - base; else ((int32_t *)oo)[i] = ((const int32_t *)off)[i] - (int32_t)base;
        }
        void *od = std::malloc((size_t)(end - base > 0 ? end - base : 1));
        if (end > base) std::memcpy(od, (const uint8_t *)src->buffers[2] + base, (size_t)(end - base));
        p->bufs.push_back(oo); p->bufs.push_back(od); p->ptrs[1] = oo; p->ptrs[2] = od; nb = 3;
    } else if (!std::strcmp(f, "b")) {
        uint8_t *ob = (uint8_t *)std::calloc((size_t)(n + 7) / 8 + 1, 1);
        const uint8_t *v = (const uint8_t *)src->buffers[1];
        for (int64_t i = 0; i < n; i++) { const int64_t j = i + o; if ((v[j >> 3] >> (j & 7)) & 1) ob[i >> 3] |= (uint8_t)(1u << (i & 7)); }
        p->bufs.push_back(ob); p->ptrs[1] = ob;
    } else {
        const uint32_t w = fixed_width(f);
        if (!w) { delete p; return false; }
        void *ov = std::malloc((size_t)(n ? n : 1) * w);
        if (n) std::memcpy(ov, (const uint8_t *)src->buffers[1] + (size_t)o * w, (size_t)n * w);
        p->bufs.push_back(ov); p->ptrs[1] = ov;
    }
    int64_t nulls = 0;
    if (src->n_buffers > 0 && src->buffers[0] && null_count(src) > 0) {
        uint8_t *bm = (uint8_t *)std::calloc((size_t)(n + 7) / 8 + 1, 1);
        const uint8_t *v = (const uint8_t *)src->buffers[0];
        for (int64_t i = 0; i < n; i++) { const int64_t j = i + o; if ((v[j >> 3] >> (j & 7)) & 1) bm[i >> 3] |= (uint8_t)(1u << (i & 7)); else nulls++; }
        p->bufs.push_back(bm); p->ptrs[0] = bm;
    }
    dst->length = n; dst->null_count = nulls; dst->n_buffers = nb; dst->buffers = p->ptrs; dst->private_data = p; dst->release = release_array;
    return true;
}

void finish_array(ArrowArray *a, OutPriv *p, int64_t n, const uint8_t *valid_bytes, int n_buffers)
{
    uint8_t *bm = (uint8_t *)std::calloc((size_t)(n + 7) / 8 + 1, 1);
    int64_t nulls = 0;
    for (int64_t i = 0; i < n; i++) { if (valid_bytes[i]) bm[i >> 3] |= (uint8_t)(1u << (i & 7)); else nulls++; }
    p->bufs.push_back(bm);
    p->ptrs[0] = nulls ? bm : nullptr;
    a->length = n; a->null_count = nulls; a->n_buffers = n_buffers; a->buffers = p->ptrs; a->private_data = p; a->release = release_array;
}

}  // namespace

extern "C" int brh_take(brh_session *s, const ArrowArray *column, const ArrowSchema *column_schema,
                        const ArrowArray *idx, const ArrowSchema *idx_schema, ArrowArray *out, ArrowSchema *out_schema)
{
    if (!s) return 1;
    if (!column || !column_schema || !idx || !idx_schema || !out || !out_schema) return fail(s, "take: null argument");
    if (std::strcmp(idx_schema->format, "I")) return fail(s, "take: the index array must be UInt32, got " + std::string(idx_schema->format));
    const char *f = column_schema->format;
    const int64_t n = idx->length;
    // indices: nulls become IVX_NULL_IDX (nearest.rs:462: left index with a null buffer)
    std::vector<uint32_t> ix((size_t)(n ? n : 1));
    {
        const uint32_t *iv = (const uint32_t *)idx->buffers[1] + idx->offset;
        const uint8_t *vb = (idx->n_buffers > 0 && idx->buffers[0] && null_count(idx) > 0) ? (const uint8_t *)idx->buffers[0] : nullptr;
        for (int64_t i = 0; i < n; i++) {
            const int64_t j = i + idx->offset;
            ix[i] = (vb && !((vb[j >> 3] >> (j & 7)) & 1)) ? IVX_NULL_IDX : iv[i];
        }
    }
    std::vector<uint8_t> vstore, valid((size_t)(n ? n : 1));
    const uint8_t *svb = rebased_validity(column, &vstore);
    const uint64_t n_src = (uint64_t)column->length;
    std::memset(out, 0, sizeof *out);
    const bool str32 = !std::strcmp(f, "u") || !std::strcmp(f, "z"), str64 = !std::strcmp(f, "U") || !std::strcmp(f, "Z");
    const bool is_struct = !std::strcmp(f, "+s"), is_list = !std::strcmp(f, "+l") || !std::strcmp(f, "+m"), is_llist = !std::strcmp(f, "+L"),
               is_fsl = !std::strncmp(f, "+w:", 3);
    if (is_struct || is_list || is_llist || is_fsl) {
        // nested columns (arrow's take handles any type, interval_join.rs:1655-1667): the row selection of a struct is the same
        // take on every child; a list's rows become ranges of child elements, i.e. one more index array for a take on the
        // child.  The leaves end in the device gathers below; offsets and validity of the nesting levels are host work.
        for (int64_t i = 0; i < n; i++) {
            if (ix[i] != IVX_NULL_IDX && ix[i] >= n_src) return fail(s, "take: index " + std::to_string(ix[i]) + " out of range (column has " + std::to_string(n_src) + " rows)");
            valid[i] = ix[i] != IVX_NULL_IDX && (!svb || ((svb[ix[i] >> 3] >> (ix[i] & 7)) & 1));
        }
        const int64_t nchild = column->n_children;
        if (nchild != column_schema->n_children || (!is_struct && nchild != 1)) return fail(s, "take: malformed nested column");
        OutPriv *p = new OutPriv();
        ArrowSchema **cschemas = (ArrowSchema **)std::calloc((size_t)(nchild ? nchild : 1), sizeof(ArrowSchema *));
        auto cleanup = [&](int64_t upto) {
            for (int64_t c = 0; c < upto; c++) { if (cschemas[c]->release) cschemas[c]->release(cschemas[c]); std::free(cschemas[c]); }
            std::free(cschemas);
            for (ArrowArray *c : p->children) { if (c->release) c->release(c); std::free(c); }
            for (void *b : p->bufs) std::free(b);
            delete p;
        };
        // the child rows to take, as a UInt32 index array with nulls
        std::vector<uint32_t> cidx; std::vector<uint8_t> cvalid_bits;
        int n_buffers = 1;
        if (is_struct) {
            cidx = ix;                                              // (null indices stay null; rows under a null struct are taken as they are)
        } else if (is_fsl) {
            const int64_t w = std::atoll(f + 3);
            if (w < 0 || (uint64_t)(column->offset + (int64_t)n_src) * (uint64_t)w >= 0xFFFFFFFFull) { cleanup(0); return fail(s, "take: fixed-size list child too large for 32-bit indices"); }
            cidx.resize((size_t)((n * w) > 0 ? n * w : 1));
            for (int64_t i = 0; i < n; i++)
                for (int64_t j = 0; j < w; j++) cidx[(size_t)(i * w + j)] = ix[i] == IVX_NULL_IDX ? IVX_NULL_IDX : (uint32_t)((column->offset + (int64_t)ix[i]) * w + j);
        } else {
            const size_t ow = is_llist ? 8 : 4;
            const uint8_t *off = (const uint8_t *)column->buffers[1] + (size_t)column->offset * ow;
            auto at = [&](uint64_t r) -> int64_t { return is_llist ? ((const int64_t *)off)[r] : (int64_t)((const int32_t *)off)[r]; };
            void *noff = std::malloc((size_t)(n + 1) * ow);
            int64_t run = 0;
            for (int64_t i = 0; i <= n; i++) {
                if (is_llist) ((int64_t *)noff)[i] = run; else ((int32_t *)noff)[i] = (int32_t)run;
                if (i < n && valid[i]) {
                    const int64_t a = at(ix[i]), b = at((uint64_t)ix[i] + 1);
                    for (int64_t e = a; e < b; e++) cidx.push_back((uint32_t)e);
                    if ((uint64_t)b >= 0xFFFFFFFFull) { std::free(noff); cleanup(0); return fail(s, "take: list child too large for 32-bit indices"); }
                    run += b - a;
                }
            }
            if (!is_llist && run > INT32_MAX) { std::free(noff); cleanup(0); return fail(s, "take: the gathered lists overflow 32-bit offsets"); }
            p->bufs.push_back(noff); p->ptrs[1] = noff; n_buffers = 2;
            if (cidx.empty()) cidx.push_back(0);
        }
        const int64_t n_cidx = is_struct ? n : is_fsl ? n * std::atoll(f + 3) : ((!is_llist) ? (int64_t)((const int32_t *)p->ptrs[1])[n] : ((const int64_t *)p->ptrs[1])[n]);
        // a UInt32 Arrow array over cidx (nulls where IVX_NULL_IDX)
        cvalid_bits.assign((size_t)(n_cidx + 7) / 8 + 1, 0);
        int64_t cnulls = 0;
        for (int64_t i = 0; i < n_cidx; i++) { if (cidx[(size_t)i] != IVX_NULL_IDX) cvalid_bits[(size_t)i >> 3] |= (uint8_t)(1u << (i & 7)); else cnulls++; }
        const void *cbufs[2] = {cnulls ? (const void *)cvalid_bits.data() : nullptr, cidx.data()};
        ArrowArray cia; std::memset(&cia, 0, sizeof cia);
        cia.length = n_cidx; cia.null_count = cnulls; cia.n_buffers = 2; cia.buffers = cbufs;
        for (int64_t c = 0; c < nchild; c++) {
            ArrowArray cc = *column->children[c];                   // (a shallow view: nothing of it is released here)
            if (is_struct) { cc.offset += column->offset; cc.length = column->length; cc.null_count = -1; }
            ArrowArray *co = (ArrowArray *)std::malloc(sizeof(ArrowArray));
            cschemas[c] = (ArrowSchema *)std::malloc(sizeof(ArrowSchema));
            if (brh_take(s, &cc, column_schema->children[c], &cia, idx_schema, co, cschemas[c])) { std::free(co); std::free(cschemas[c]); cleanup(c); return 1; }
            // the child's field keeps its own name and nullability
            cschemas[c]->flags = column_schema->children[c]->flags;
            p->children.push_back(co);
        }
        finish_array(out, p, n, valid.data(), n_buffers);
        out->n_children = nchild;
        out->children = p->children.data();
        make_schema(out_schema, f, column_schema->name ? column_schema->name : "", true);
        out_schema->flags |= column_schema->flags & 4;              // ARROW_FLAG_MAP_KEYS_SORTED
        out_schema->n_children = nchild; out_schema->children = cschemas;
        return 0;
    }
    if (column_schema->dictionary) {
        // dictionary-encoded column (arrow's take gathers the keys and keeps the dictionary): the keys are a fixed-width
        // gather on the device, the output carries an owned copy of the dictionary values
        const uint32_t w = fixed_width(f);
        if (!w || !column->dictionary) return fail(s, "take: malformed dictionary column");
        ArrowArray *dict = (ArrowArray *)std::malloc(sizeof(ArrowArray));
        if (!copy_flat_array(column->dictionary, column_schema->dictionary->format, dict)) {
            std::free(dict);
            return fail(s, "take: unsupported dictionary value type " + std::string(column_schema->dictionary->format) + " (flat value types only)");
        }
        const uint8_t *src = (const uint8_t *)column->buffers[1] + (size_t)column->offset * w;
        void *o = std::malloc((size_t)(n ? n : 1) * w);
        const ivx_status st = ivx_take_fixed(s->ctx, IVX_MEM_HOST, src, w, n_src, svb, ix.data(), (uint64_t)n, o, valid.data());
        if (st != IVX_OK) { std::free(o); dict->release(dict); std::free(dict); return fail_ivx(s, st); }
        OutPriv *p = new OutPriv();
        p->bufs.push_back(o);
        p->ptrs[1] = o;
        p->dict = dict;
        finish_array(out, p, n, valid.data(), 2);
        out->dictionary = dict;
        make_schema(out_schema, f, column_schema->name ? column_schema->name : "", true);
        out_schema->flags |= column_schema->flags & 1;              // ARROW_FLAG_DICTIONARY_ORDERED
        out_schema->dictionary = (ArrowSchema *)std::malloc(sizeof(ArrowSchema));
        make_schema(out_schema->dictionary, column_schema->dictionary->format, column_schema->dictionary->name ? column_schema->dictionary->name : "",
                    (column_schema->dictionary->flags & 2) != 0);
        return 0;
    }
    if (str32 || str64) {
        const size_t ow = str64 ? 8 : 4;
        const uint8_t *off = (const uint8_t *)column->buffers[1] + (size_t)column->offset * ow;
        // the data buffer is addressed by absolute offsets, so it goes over whole: up to the last offset of the slice
        const uint64_t nbytes = str64 ? (uint64_t)((const int64_t *)off)[n_src] : (uint64_t)((const int32_t *)off)[n_src];
        void *ooff = std::malloc((size_t)(n + 1) * ow);
        uint64_t need = 0;
        ivx_status st = ivx_take_utf8(s->ctx, IVX_MEM_HOST, str64, off, (const uint8_t *)column->buffers[2], n_src, nbytes, svb, ix.data(), (uint64_t)n,
                                      ooff, nullptr, 0, &need, valid.data());
        uint8_t *odata = (uint8_t *)std::malloc((size_t)(need ? need : 1));
        if (st == IVX_OK)
            st = ivx_take_utf8(s->ctx, IVX_MEM_HOST, str64, off, (const uint8_t *)column->buffers[2], n_src, nbytes, svb, ix.data(), (uint64_t)n,
                               ooff, odata, need ? need : 1, &need, valid.data());
        if (st != IVX_OK) { std::free(ooff); std::free(odata); return fail_ivx(s, st); }
        OutPriv *p = new OutPriv();
        p->bufs.push_back(ooff); p->bufs.push_back(odata);
        p->ptrs[1] = ooff; p->ptrs[2] = odata;
        finish_array(out, p, n, valid.data(), 3);
    } else if (!std::strcmp(f, "vu") || !std::strcmp(f, "vz")) {   // Utf8View / BinaryView (DataFusion's default string type for Parquet)
        if (column->n_buffers < 3) return fail(s, "take: malformed view array");
        const uint32_t nb = (uint32_t)(column->n_buffers - 3);
        const int64_t *sizes = (const int64_t *)column->buffers[column->n_buffers - 1];
        std::vector<const uint8_t *> bufs(nb ? nb : 1, nullptr); std::vector<uint64_t> bytes(nb ? nb : 1, 0);
        for (uint32_t b = 0; b < nb; b++) { bufs[b] = (const uint8_t *)column->buffers[2 + b]; bytes[b] = (uint64_t)sizes[b]; }
        const uint8_t *views = (const uint8_t *)column->buffers[1] + (size_t)column->offset * 16;
        void *oviews = std::malloc((size_t)(n ? n : 1) * 16);
        uint64_t need = 0;
        ivx_status st = ivx_take_view(s->ctx, IVX_MEM_HOST, views, bufs.data(), bytes.data(), nb, n_src, svb, ix.data(), (uint64_t)n,
                                      nullptr, nullptr, 0, &need, valid.data());
        uint8_t *odata = (uint8_t *)std::malloc((size_t)(need ? need : 1));
        if (st == IVX_OK)
            st = ivx_take_view(s->ctx, IVX_MEM_HOST, views, bufs.data(), bytes.data(), nb, n_src, svb, ix.data(), (uint64_t)n,
                               oviews, odata, need ? need : 1, &need, valid.data());
        if (st != IVX_OK) { std::free(oviews); std::free(odata); return fail_ivx(s, st); }
        int64_t *osz = (int64_t *)std::malloc(sizeof(int64_t));
        osz[0] = (int64_t)need;
        OutPriv *p = new OutPriv();
        p->bufs.push_back(oviews); p->bufs.push_back(odata); p->bufs.push_back(osz);
        p->ptrs[1] = oviews; p->ptrs[2] = odata; p->ptrs[3] = osz;
        finish_array(out, p, n, valid.data(), 4);
    } else if (!std::strcmp(f, "b")) {                       // Boolean: bit-packed values
        const uint8_t *src = (const uint8_t *)column->buffers[1];
        std::vector<uint8_t> sstore;
        if (column->offset % 8) {                             // re-base the value bitmap like the validity bitmap
            sstore.assign((size_t)(column->length + 7) / 8, 0);
            for (int64_t i = 0; i < column->length; i++) { const int64_t j = i + column->offset; if ((src[j >> 3] >> (j & 7)) & 1) sstore[i >> 3] |= (uint8_t)(1u << (i & 7)); }
            src = sstore.data();
        } else src += column->offset / 8;
        uint8_t *o = (uint8_t *)std::calloc((size_t)(n + 7) / 8 + 1, 1);
        const ivx_status st = ivx_take_bits(s->ctx, IVX_MEM_HOST, src, n_src, svb, ix.data(), (uint64_t)n, o, valid.data());
        if (st != IVX_OK) { std::free(o); return fail_ivx(s, st); }
        OutPriv *p = new OutPriv();
        p->bufs.push_back(o);
        p->ptrs[1] = o;
        finish_array(out, p, n, valid.data(), 2);
    } else {
        const uint32_t w = fixed_width(f);
        if (!w) return fail(s, "take: unsupported column type " + std::string(f) + " (fixed-width primitives, Boolean, Utf8/LargeUtf8/Binary/LargeBinary and their views, dictionaries and struct / list nestings of those only)");
        const uint8_t *src = (const uint8_t *)column->buffers[1] + (size_t)column->offset * w;
        void *o = std::malloc((size_t)(n ? n : 1) * w);
        const ivx_status st = ivx_take_fixed(s->ctx, IVX_MEM_HOST, src, w, n_src, svb, ix.data(), (uint64_t)n, o, valid.data());
        if (st != IVX_OK) { std::free(o); return fail_ivx(s, st); }
        OutPriv *p = new OutPriv();
        p->bufs.push_back(o);
        p->ptrs[1] = o;
        finish_array(out, p, n, valid.data(), 2);
    }
    make_schema(out_schema, f, column_schema->name ? column_schema->name : "", true);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// IntervalJoinStream as a push interface (interval_join.rs:934-1140, :1418-1677): the build side is indexed
// once (WaitBuildSide / collect_left_input :584-700), probe RecordBatches arrive one by one (FetchProbeBatch)
// and each is joined against the index (ProcessProbeBatch).  A GPU call per 8192-row batch would be all launch
// latency, so the probe batches are COALESCED here -- what DataFusion's CoalesceBatchesExec does in front of
// an operator -- into groups of `coalesce_rows` rows; a group is probed in one count + fill pair (its columns
// cross PCIe once, ivx.h "two-call protocol") and yields ONE result: pairs (build_idx, probe_idx) with
// probe_idx counted over the group's concatenated rows, and the row offset of every batch in the group.
struct brh_join_stream {
    brh_session *s = nullptr;
    ivx_index *ix = nullptr;
    std::vector<std::string> pkeys; std::string pstart, pend;      // the probe side's column names (owned)
    std::unordered_map<std::string, uint32_t> dict;                 // build-side key -> id; unknown keys get id nk (no build rows)
    uint32_t nk = 0;
    uint64_t short_keys[1024] = {}; uint32_t short_ids[1024] = {}; uint32_t n_short = 0;   // packed short names -> id
    bool strict = false;
    uint64_t coalesce_rows = 0;
    // the open group
    std::vector<uint32_t> gk; std::vector<int32_t> gs, ge; std::vector<int64_t> goff;
    uint64_t first_batch = 0, n_pushed = 0;
    int join_type = BRH_JOIN_INNER;                                 // BRH_JOIN_* or BRH_JOIN_NEAREST (Algorithm::CoitreesNearest)
    uint64_t max_rows = 0;                                          // output rows per result (0 = a group's rows in one result)
    struct Result { uint64_t first_batch, n_batches; std::vector<uint32_t> bi, pi; std::vector<uint8_t> bvalid, pvalid; std::vector<int64_t> off; bool last; };
    std::deque<Result> ready;
    // LeftSemi / LeftAnti / Left / Full: the build side's match marks, one bit per build row, ORed into by every flushed group
    std::vector<uint32_t> marks; uint64_t nb = 0;
    bool finished = false;                                          // the build-side result behind the last group is queued
    ~brh_join_stream() { if (ix) ivx_index_free(ix); }
};

namespace {

// One group of coalesced probe batches -> one result, or -- with an output budget (the reference's low-memory
// stream, interval_join.rs:1153-1299; BIO_MAX_OUTPUT_BATCH_SIZE, :543-548) -- several: a result holds whole probe rows
// and ends after the row at which its running output-row count reaches the budget (:1199-1216, :1256-1273), so it
// stays below budget + the matches of its last row.  probe_idx always counts over the group's concatenated rows.
int stream_flush(brh_join_stream *js)
{
    brh_session *s = js->s;
    if (js->goff.empty()) return 0;
    const uint64_t np = js->gs.size();
    std::vector<int64_t> off = js->goff; off.push_back((int64_t)np);
    const uint64_t first = js->first_batch, nb = js->goff.size();
    auto emit = [&](std::vector<uint32_t> &&bi, std::vector<uint32_t> &&pi, std::vector<uint8_t> &&bv, bool last) {
        brh_join_stream::Result r;
        r.first_batch = first; r.n_batches = nb; r.off = off; r.last = last;
        r.bi = std::move(bi); r.pi = std::move(pi); r.bvalid = std::move(bv);
        js->ready.push_back(std::move(r));
    };
    const uint32_t *gk = js->gk.data(); const int32_t *gs = js->gs.data(), *ge = js->ge.data();
    ivx_status st;
    if (js->join_type == BRH_JOIN_RIGHT_SEMI || js->join_type == BRH_JOIN_RIGHT_ANTI) {          // :1014-1024, :1167-1202, :1433-1447
        std::vector<uint8_t> ex(np ? np : 1);
        st = ivx_probe_exists(s->ctx, js->ix, IVX_MEM_HOST, gk, gs, ge, np, ex.data());
        if (st != IVX_OK) return fail_ivx(s, st);
        const bool want = js->join_type == BRH_JOIN_RIGHT_SEMI;
        std::vector<uint32_t> pi;
        for (uint64_t i = 0; i < np; i++) {
            if ((ex[i] != 0) == want) pi.push_back((uint32_t)i);
            if (js->max_rows && pi.size() >= js->max_rows && i + 1 < np) { emit({}, std::move(pi), {}, false); pi.clear(); }
        }
        emit({}, std::move(pi), {}, true);
    } else if (js->join_type == BRH_JOIN_NEAREST) {                                              // :864-870, :1226-1238: one row per probe row
        std::vector<uint32_t> bi(np ? np : 1), pi(np ? np : 1);
        uint64_t rows = 0;
        st = ivx_probe_nearest(s->ctx, js->ix, IVX_MEM_HOST, gk, gs, ge, np, 0, 1, 1, bi.data(), pi.data(), nullptr, np, &rows);
        if (st != IVX_OK) return fail_ivx(s, st);
        const uint64_t step = js->max_rows ? js->max_rows : (rows ? rows : 1);
        for (uint64_t a = 0; a < rows || a == 0; a += step) {
            const uint64_t b = std::min(rows, a + step);
            std::vector<uint32_t> sb(bi.begin() + a, bi.begin() + b), sp(pi.begin() + a, pi.begin() + b);
            std::vector<uint8_t> bv(b - a);
            for (uint64_t i = 0; i < b - a; i++) { bv[i] = sb[i] != IVX_NULL_IDX; if (!bv[i]) sb[i] = 0; }   // NULL build row (u32::MAX marker, :1233)
            emit(std::move(sb), std::move(sp), std::move(bv), b >= rows);
            if (b >= rows) break;
        }
    } else if (js->join_type == BRH_JOIN_LEFT_SEMI || js->join_type == BRH_JOIN_LEFT_ANTI) {     // marks only: the group gives no result
        st = ivx_probe_mark_build(s->ctx, js->ix, IVX_MEM_HOST, gk, gs, ge, np, js->marks.data());
        if (st != IVX_OK) return fail_ivx(s, st);
    } else if (join_marks_build(js->join_type)) {                                                // Left / Right / Full (regular mode only)
        std::vector<uint32_t> bi, pi; std::vector<uint8_t> bv;
        uint64_t n_pairs = 0;
        if (join_pairs(s, js->ix, gk, gs, ge, np, join_null_build(js->join_type), &bi, &pi, &bv, &n_pairs)) return 1;
        if (join_null_probe(js->join_type)) {
            st = ivx_bits_mark(s->ctx, IVX_MEM_HOST, bi.data(), n_pairs, js->marks.data(), js->nb);
            if (st != IVX_OK) return fail_ivx(s, st);
        }
        emit(std::move(bi), std::move(pi), std::move(bv), true);
    } else if (!js->max_rows) {
        uint64_t total = 0, written = 0;
        st = ivx_probe_overlap_count(s->ctx, js->ix, IVX_MEM_HOST, gk, gs, ge, np, nullptr, &total);
        if (st != IVX_OK) return fail_ivx(s, st);
        std::vector<uint32_t> bi(total ? total : 1), pi(total ? total : 1);
        st = ivx_probe_overlap_fill(s->ctx, js->ix, IVX_MEM_HOST, gk, gs, ge, np, bi.data(), pi.data(), total, &written);
        if (st != IVX_OK) return fail_ivx(s, st);
        bi.resize(written); pi.resize(written);
        emit(std::move(bi), std::move(pi), {}, true);
    } else {
        // rle_right of the whole group first (ONE device call), then the pairs slice by slice of probe rows
        std::vector<uint32_t> rle(np ? np : 1);
        uint64_t total = 0;
        st = ivx_probe_overlap_count(s->ctx, js->ix, IVX_MEM_HOST, gk, gs, ge, np, rle.data(), &total);
        if (st != IVX_OK) return fail_ivx(s, st);
        uint64_t r0 = 0;
        while (r0 < np || r0 == 0) {
            uint64_t r1 = r0, sum = 0;
            while (r1 < np && sum < js->max_rows) sum += rle[r1++];       // ends after the row that reaches the budget
            if (total - sum == 0 || r1 >= np) {                            // nothing but matchless rows behind it: this is the last result
                for (; r1 < np; r1++) sum += rle[r1];
            }
            std::vector<uint32_t> bi(sum ? sum : 1), pi(sum ? sum : 1);
            uint64_t written = 0;
            if (sum) {
                st = ivx_probe_overlap_fill(s->ctx, js->ix, IVX_MEM_HOST, gk + r0, gs + r0, ge + r0, r1 - r0, bi.data(), pi.data(), sum, &written);
                if (st != IVX_OK) return fail_ivx(s, st);
                if (written != sum) return fail(s, "join stream: a slice's pair count changed between the count and the fill call");
                for (uint64_t i = 0; i < written; i++) pi[i] += (uint32_t)r0;
            }
            bi.resize(written); pi.resize(written);
            total -= sum;
            emit(std::move(bi), std::move(pi), {}, r1 >= np);
            r0 = r1;
            if (r0 >= np) break;
        }
    }
    js->first_batch = js->n_pushed;
    js->gk.clear(); js->gs.clear(); js->ge.clear(); js->goff.clear();
    return 0;
}

}  // namespace

extern "C" int brh_join_stream_open(brh_session *s, brh_batch build, brh_columns bcols, brh_columns pcols, int strict_predicate,
                                    uint64_t coalesce_rows, int join_type, uint64_t max_output_rows, brh_join_stream **out)
{
    if (!s || !out) return 1;
    *out = nullptr;
    if (join_type < BRH_JOIN_INNER || join_type > BRH_JOIN_FULL) return fail(s, "join stream: unsupported join type");
    if (join_marks_build(join_type) && max_output_rows != 0)
        return fail(s, "join stream: max_output_rows > 0 (the low-memory mode) is not supported with LeftSemi / LeftAnti / Left / Right / Full joins");
    if (max_output_rows == BRH_MAX_OUTPUT_ENV) {                  // the reference's low-memory default (interval_join.rs:543-548)
        // usize::from_str: an optional '+', then digits only, no overflow; anything else is the default.  A parsed 0 is kept by
        // the reference (it then emits after every probe row); here 0 already means "regular mode", so 0 becomes 1: one
        // output row per batch is the smallest budget there is.
        const char *e = std::getenv("BIO_MAX_OUTPUT_BATCH_SIZE");
        max_output_rows = 100000;
        if (e) {
            const char *p = e + (*e == '+');
            unsigned long long v = 0; bool ok = *p != 0;
            for (; ok && *p; p++) {
                if (*p < '0' || *p > '9' || v > (~0ull - (unsigned)(*p - '0')) / 10) ok = false;
                else v = v * 10 + (unsigned)(*p - '0');
            }
            if (ok) max_output_rows = v ? v : 1;
        }
    }
    if (pcols.n_keys != bcols.n_keys || pcols.n_keys < 1) return fail(s, "both sides need the same number (>= 1) of key columns");
    KeyDict kd; Side32 B;
    if (build_keys(s, {{build, bcols}}, &kd, true) || load_side32(s, build, bcols, &B)) return 1;
    if (strict_predicate) for (auto &v : B.e) v = (int32_t)((uint32_t)v - 1u);          // intervals.rs:85-115
    std::unique_ptr<brh_join_stream> js(new brh_join_stream());
    js->s = s; js->strict = strict_predicate != 0;
    js->join_type = join_type; js->max_rows = max_output_rows;
    js->coalesce_rows = coalesce_rows ? coalesce_rows : (4u << 20);
    js->nk = (uint32_t)kd.names.size();
    for (uint32_t i = 0; i < js->nk; i++) js->dict.emplace(kd.names[i], i);
    for (int k = 0; k < pcols.n_keys; k++) js->pkeys.emplace_back(pcols.keys[k]);
    js->pstart = pcols.start; js->pend = pcols.end;
    // one key id more than the build side has: "contig the build side does not know", never matches
    ivx_status st = ivx_index_build(s->ctx, join_type == BRH_JOIN_NEAREST ? IVX_KIND_NEAREST : IVX_KIND_OVERLAP, IVX_MEM_HOST, kd.ids[0].data(),
                                    B.s.data(), B.e.data(), B.s.size(), js->nk + 1, &js->ix);
    if (st != IVX_OK) return fail_ivx(s, st);
    js->nb = B.s.size();
    if (join_marks_build(join_type)) js->marks.assign((js->nb + 31) / 32 + 1, 0u);
    *out = js.release();
    return 0;
}

extern "C" int brh_join_stream_push(brh_join_stream *js, brh_batch probe, int *n_ready)
{
    if (!js) return 1;
    brh_session *s = js->s;
    std::vector<const char *> keyp;
    for (auto &k : js->pkeys) keyp.push_back(k.c_str());
    const brh_columns pc{keyp.data(), (int)keyp.size(), js->pstart.c_str(), js->pend.c_str()};
    std::vector<StrCol> cols(pc.n_keys);
    for (int k = 0; k < pc.n_keys; k++) if (get_contig(s, probe, pc.keys[k], &cols[k])) return 1;
    Side32 P;
    if (load_side32(s, probe, pc, &P)) return 1;
    const int64_t n = probe.array->length;
    const size_t base = js->gs.size();
    js->goff.push_back((int64_t)base);
    js->gk.resize(base + (size_t)n); js->gs.resize(base + (size_t)n); js->ge.resize(base + (size_t)n);
    // key ids.  Rows of one contig come in runs (coordinate-sorted files), so the previous row's answer is tried
    // first; names of up to 7 bytes ("chr1" ... "chrUn") are looked up as one packed 64-bit word in a small
    // open-addressing table (short_ids, filled as names are met), anything longer in the string dictionary
    std::string scratch, last; uint32_t last_id = 0; bool have_last = false; uint64_t last_packed = 0;
    for (int64_t i = 0; i < n; i++) {
        std::string_view k;
        if (cols.size() == 1) k = cols[0].null_at(i) ? NULL_KEY : cols[0].at(i);
        else { scratch.clear(); for (size_t c = 0; c < cols.size(); c++) { if (c) scratch.push_back('\x1f'); scratch.append(cols[c].null_at(i) ? NULL_KEY : cols[c].at(i)); } k = scratch; }
        if (k.size() <= 7) {
            uint64_t packed = 0;
            std::memcpy(&packed, k.data(), k.size());
            packed |= (uint64_t)(k.size() + 1) << 56;                    // never 0: 0 marks an empty slot
            if (packed != last_packed) {
                bool hit = false;
                uint32_t h = (uint32_t)((packed * 0x9E3779B97F4A7C15ull) >> 54);
                for (;; h = (h + 1) & 1023u) {
                    if (js->short_keys[h] == packed) { last_id = js->short_ids[h]; hit = true; break; }
                    if (js->short_keys[h] == 0) break;
                }
                if (!hit) {
                    auto it = js->dict.find(std::string(k));
                    last_id = it == js->dict.end() ? js->nk : it->second;
                    if (js->n_short < 512) { js->short_keys[h] = packed; js->short_ids[h] = last_id; js->n_short++; }   // h = the empty slot found
                }
                last_packed = packed; have_last = false;
            }
        } else if (!have_last || k != std::string_view(last)) {
            last.assign(k.data(), k.size());
            auto it = js->dict.find(last);
            last_id = it == js->dict.end() ? js->nk : it->second;
            have_last = true; last_packed = 0;
        }
        js->gk[base + (size_t)i] = last_id;
        js->gs[base + (size_t)i] = P.s[(size_t)i];
        js->ge[base + (size_t)i] = js->strict ? (int32_t)((uint32_t)P.e[(size_t)i] - 1u) : P.e[(size_t)i];
    }
    js->n_pushed++;
    if (js->gs.size() >= js->coalesce_rows && stream_flush(js)) return 1;
    if (n_ready) *n_ready = (int)js->ready.size();
    return 0;
}

extern "C" int brh_join_stream_finish(brh_join_stream *js, int *n_ready)
{
    if (!js) return 1;
    if (stream_flush(js)) return 1;
    if (join_marks_build(js->join_type) && !js->finished) {
        // behind the last group: the build-side rows (matched: LeftSemi; unmatched: LeftAnti / Left / Full; Right has none)
        brh_join_stream::Result r;
        r.first_batch = js->n_pushed; r.n_batches = 0; r.off = {0}; r.last = true;
        if (js->join_type != BRH_JOIN_RIGHT && select_build_rows(js->s, js->marks, js->nb, js->join_type == BRH_JOIN_LEFT_SEMI, &r.bi)) return 1;
        if (js->join_type == BRH_JOIN_RIGHT) r.bi.clear();
        if (join_null_probe(js->join_type)) { r.pi.assign(r.bi.size(), 0u); r.pvalid.assign(r.bi.size(), 0); }
        if (join_null_build(js->join_type)) r.bvalid.assign(r.bi.size(), 1);
        js->ready.push_back(std::move(r));
        js->finished = true;
    }
    if (n_ready) *n_ready = (int)js->ready.size();
    return 0;
}

extern "C" int brh_join_stream_next(brh_join_stream *js, uint64_t *first_batch, uint64_t *n_batches, int *group_done,
                                    ArrowArray *build_idx, ArrowSchema *build_idx_schema, ArrowArray *probe_idx, ArrowSchema *probe_idx_schema,
                                    ArrowArray *batch_offsets, ArrowSchema *batch_offsets_schema)
{
    if (!js) return 1;
    if (js->ready.empty()) return fail(js->s, "join stream: no result is ready");
    brh_join_stream::Result &r = js->ready.front();
    if (first_batch) *first_batch = r.first_batch;
    if (n_batches) *n_batches = r.n_batches;
    if (group_done) *group_done = r.last ? 1 : 0;
    const bool nullable = js->join_type == BRH_JOIN_NEAREST || join_null_build(js->join_type);
    const bool pnullable = join_null_probe(js->join_type);          // (a result without a validity vector has no NULLs: a group's pairs)
    make_primitive<uint32_t>(build_idx, r.bi.data(), (int64_t)r.bi.size(), nullable && !r.bvalid.empty() ? r.bvalid.data() : nullptr); make_schema(build_idx_schema, "I", "build_idx", nullable);
    make_primitive<uint32_t>(probe_idx, r.pi.data(), (int64_t)r.pi.size(), pnullable && !r.pvalid.empty() ? r.pvalid.data() : nullptr); make_schema(probe_idx_schema, "I", "probe_idx", pnullable);
    make_primitive<int64_t>(batch_offsets, r.off.data(), (int64_t)r.off.size(), nullptr); make_schema(batch_offsets_schema, "l", "batch_offsets", false);
    js->ready.pop_front();
    return 0;
}

extern "C" void brh_join_stream_close(brh_join_stream *js) { delete js; }
