/*
 * fugu_host.h -- the host side of fugu's search path above the device ABI
 * (include/fugu.h), written in C++ because the reference's toolchain (Rust)
 * is absent.  It mirrors, name for name, the reference pieces
 * around the replaced call:
 *
 *   fg_db_*            DatasetManager (src/db/config.rs:91-331): namespace
 *                      registry; create/delete are the routes the CLI speaks
 *                      but the server lacks (cli.rs:241-243, 280-282)
 *   fg_db_upsert_record NamedIndex::upsert for the docs index
 *                      (src/db/document.rs:23-67, build_full_document :116-184):
 *                      ObjectRecord::validate (src/object.rs:31-78), delete by
 *                      the RAW id term, index `text`, metadata["name"] and the
 *                      facets (get_all_facet_paths, document.rs:277-309)
 *   fg_db_upsert       the same with `name` given directly (no namespace facets)
 *   fg_db_commit       IndexWriter::commit + reader reload: rebuilds the
 *                      namespace's immutable device snapshot (fg_index)
 *   fg_db_add_file     POST /add/{namespace} (cli.rs:392-397, types.rs:71-75)
 *   fg_db_search_ex    Dataset::search (src/db/search.rs:74-218): QueryParser
 *                      over [text, name], facet filters (build_facet_query,
 *                      :221-324), TopDocs::with_limit(offset+per_page) on the
 *                      GPU, doc fetch, skip(offset).take(per_page)
 *   fg_db_search_json  perform_search (src/server/handlers/search.rs:350-402)
 *                      + the response shapes of the GET /search, POST /search
 *                      and POST /search/{namespace} handlers (Appendix B)
 *   fg_analyze         the "default" analyzer (SimpleTokenizer ->
 *                      RemoveLongFilter(40) -> LowerCaser)
 *   fg_parse_query     the QueryParser subset the device runs
 *   fg_parse_query_clauses  the same as clauses: terms, and phrases with offsets
 *
 * Phrase queries run on the device (k_phrase, slop 0): a word the analyzer
 * splits into several tokens (`e-mail`, `user@example.com`, `3.14`) or a quoted
 * literal ("new york"), when the phrase is the query's only clause and no facet
 * filter is given (segments built with FUGU_POSITIONS=0 keep no positions and
 * refuse them).  With fg_phrase_clauses(1) (fugu.h; process-wide, off by
 * default) a phrase may also stand beside other clauses (`e-mail server`,
 * `+e-mail -spam`, `"new york" pizza`: k_bphrase); fg_db_search* then run such
 * queries as they are.  With fg_group_clauses(1) (fugu.h; process-wide, off by
 * default) one level of grouping over plain single-token words is in the subset
 * too (k_group): a parenthesised group where a word may stand -- `(a b)` /
 * `(a OR b)` any-of, `(a AND b)` / `(+a +b)` all-of; bare, behind `+` / `-`, or
 * an operand of the uniform AND / OR forms -- and mixed infix `a AND b OR c`,
 * where AND binds tighter.  fg_parse_query_clauses prints a group as
 * "<occur>:(a | b)" or "<occur>:(a & b)"; fg_parse_query and fg_parse_query_occur
 * refuse one, and so do the count entry points (fg_db_facet_counts,
 * fg_db_facet_tree, fg_db_facets_json) unless fg_count_clauses(1) is set (fugu.h;
 * process-wide, off by default), with which they count phrase and group queries
 * as fg_db_search* run them.  Queries outside the device subset
 * (grouping while that switch is off or deeper than one level, a phrase beside other
 * clauses while that switch is off, a group beside a phrase -- `e-mail (server OR host)`
 * -- unless fg_group_phrase_clauses(1) is set as well (fugu.h; process-wide, off by
 * default: k_gphrase), a phrase as a group member -- `(e-mail OR email) server`,
 * `e-mail AND server OR host` -- unless fg_group_member_phrases(1) is set as well
 * (fugu.h; process-wide, off by default: k_mgroup), a phrase or a group with filters unless
 * fg_filter_clauses(1) is set (fugu.h; process-wide, off by default), slop / prefix
 * suffixes on a quoted literal, field: -- unless fg_field_clauses(1) is set (fugu.h;
 * process-wide, off by default: k_field), with which `text:WORD` / `name:WORD`, WORD a
 * plain word of one token, is that field's TermQuery; fg_parse_query_clauses prints it
 * "<occur>:name:report@0", fg_parse_query and fg_parse_query_occur refuse it, and so do
 * the count entry points; with fg_field_phrases(1) on top of it (fugu.h; process-wide,
 * off by default: k_fphrase) WORD may analyze to several tokens or be a plain quoted
 * literal, that field's PhraseQuery (`name:"annual report"`, `name:e-mail`, printed
 * "<occur>:name:annual@0 report@1"; a quoted literal of one token is a field term), and
 * a field term may stand beside a phrase clause --,
 * boosts, a text query with filters that parse to no facet term) return
 * FG_EUNSUPPORTED: the reference host then runs tantivy; this library never
 * answers them on the CPU.  Empty queries (AllQuery), facet-only queries and
 * text + facet filters run on the device.
 */
#ifndef FUGU_HOST_H
#define FUGU_HOST_H

#include "fugu.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fg_db fg_db;

#define FG_ENOTFOUND (-6) /* namespace not found: "Namespace '...' not found" */
#define FG_EEXIST (-7)    /* namespace already exists */

/* Response shapes. */
/* Every response is a serde_json Value in the reference, so object keys come out
 * in byte order (serde_json without preserve_order, Cargo.lock:4313-4322), and
 * stored metadata is re-serialized the same way (sorted keys, serde numbers). */
#define FG_SHAPE_GET_SEARCH 0  /* GET /search: {page, per_page, query, results, total}, text stripped unless asked */
#define FG_SHAPE_POST_SEARCH 1 /* POST /search, POST /search/{namespace}: {filters, page, per_page, query,
                                * results, status, total}, text kept, no per_page clamp */
#define FG_SHAPE_GET_SEARCH_PATH 2 /* GET /search/{query} (handlers/search.rs:79-139): `query` is the URL-encoded
                                    * path component (decoded here; bad UTF-8 -> 400 "Invalid URL encoding in
                                    * query", FG_EINVAL); page 0, per_page 20 */

/* ctx may be NULL: the registry, upserts and doc store then work on the host
 * alone and fg_db_commit fails with FG_ENODEV (CPU tests of the host logic). */
int fg_db_create(fg_ctx* ctx, int dev, const char* default_namespace, fg_db** out);
int fg_db_destroy(fg_db* db);
int fg_db_namespace_create(fg_db* db, const char* name);
int fg_db_namespace_delete(fg_db* db, const char* name);
/* {"namespaces":[...],"status":"success"} (handlers/namespaces.rs:24-30), names sorted */
int fg_db_namespaces_json(fg_db* db, char* out, size_t cap, size_t* len);

/* ObjectRecord (src/object.rs:8-27) as the upsert routes receive it. */
typedef struct fg_object_record {
  const char* id;
  const char* text;
  const char* metadata_json;    /* a JSON object, or NULL (metadata: None) */
  const char* namespace_;       /* ObjectRecord.namespace, or NULL */
  const char* organization;     /* or NULL */
  const char* conversation_id;  /* or NULL */
  const char* data_type;        /* or NULL */
  const char* const* facets;    /* ObjectRecord.facets: n_facets paths when has_facets */
  uint32_t n_facets;
  int has_facets;               /* Some(facets) (even empty) vs None */
} fg_object_record;
int fg_db_upsert_record(fg_db* db, const char* ns, const fg_object_record* rec);
/* POST /batch/upsert (src/server/handlers/ingest.rs:160-220, Dataset::
 * batch_upsert src/db/document.rs:70-73): n records {id, text} (no metadata,
 * namespace or facets) as two byte buffers with offsets [n+1]; every record is
 * validated before any is upserted, then one commit (one segment), as
 * NamedIndex::upsert commits once per call (src/db/document.rs:65). */
int fg_db_upsert_batch(fg_db* db, const char* ns, uint32_t n, const char* ids, const uint64_t* id_off,
                       const char* texts, const uint64_t* text_off);
int fg_db_upsert(fg_db* db, const char* ns, const char* id, const char* text, const char* name,
                 const char* metadata_json);
/* IndexWriter::commit (src/db/document.rs:65): the docs since the last commit
 * become a segment, the older segments are rescored with the new statistics
 * and pick up the deletes of the upserts since the last commit (a delete takes
 * effect at the commit, as delete_term does; a merge in between neither drops
 * nor flags the doc).  When 8 segments of one size level have accumulated
 * (tantivy's LogMergePolicy) the namespace is queued for the background merger:
 * the run becomes one segment, built and rescored off the commit path and
 * swapped in between commits; readers keep the snapshot they hold. */
int fg_db_commit(fg_db* db, const char* ns);
/* Block until no merge of the namespace is queued or running (tests, shutdown);
 * FG_EHIP with the message when a background merge failed. */
int fg_db_merge_wait(fg_db* db, const char* ns);
typedef struct fg_merge_info {
  uint64_t merges;           /* merges done */
  uint64_t merged_docs;      /* alive docs written by them */
  double merge_ms_total, merge_ms_last, merge_ms_max;
  uint32_t segments;         /* segments of the current snapshot */
  int pending;               /* a merge is queued or running */
  uint64_t n_docs_stats;     /* the namespace's BM25 statistics: N (deleted-not-merged included) */
  uint64_t tot_tokens[2];    /* total_num_tokens(text), (name) */
  uint64_t tot_facet_tokens; /* total_num_tokens(facet) */
} fg_merge_info;
int fg_db_merge_info_get(fg_db* db, const char* ns, fg_merge_info* out);
/* The merge policy alone (host only): given the namespace's segments in doc
 * order (their doc counts), the contiguous run [*j0, *j1) the merger merges
 * next, *j0 == *j1 when none (tantivy LogMergePolicy levels, contiguous runs;
 * FUGU_MERGE_MAX_DOCS = set_max_docs_before_merge, default 10M). */
int fg_merge_policy_pick(const uint64_t* seg_docs, uint32_t n_segs, uint32_t* j0, uint32_t* j1);
/* Global doc ids of segment `seg` of the current snapshot, in its doc order:
 * *n = its size, out[0..min(n, cap)) (out may be NULL). */
int fg_db_segment_docs(fg_db* db, const char* ns, uint32_t seg, uint32_t* out, uint32_t cap, uint32_t* n);
int fg_db_add_file(fg_db* db, const char* ns, const char* name, const char* body);
/* docs stored in the namespace (deleted included = tantivy max_doc) and alive ones */
int fg_db_doc_count(fg_db* db, const char* ns, uint64_t* total, uint64_t* alive);

typedef struct fg_hit {
  float score;
  uint32_t doc; /* global doc id in the namespace (insertion order) */
} fg_hit;
/* Dataset::search: hits of page `page` (per_page each), *n_out <= per_page.
 * filters: the request's `filters` strings (FuguSearchQuery / JsonQueryRequest). */
int fg_db_search_ex(fg_db* db, const char* ns, const char* query, const char* const* filters, uint32_t n_filters,
                    uint32_t page, uint32_t per_page, fg_hit* out, uint32_t cap, uint32_t* n_out);
int fg_db_search(fg_db* db, const char* ns, const char* query, uint32_t page, uint32_t per_page, fg_hit* out,
                 uint32_t cap, uint32_t* n_out);
/* Phase times of every search of the process while enabled (all threads):
 * out_ms[0..5] = parse + dictionary, host planning (+ upload queued), launches,
 * kernels + merge + D2H until the hits are on the host, JSON doc fetch +
 * serialization, the whole fg_db_search* call; *calls = fg_db_search* calls.
 * Reading resets the sums; enable: 1 on, 0 off, -1 unchanged.  Off by default
 * (one relaxed load per phase boundary). */
#define FG_SEARCH_PHASES 6
int fg_search_trace(int enable, double* out_ms, uint32_t n, uint64_t* calls);
/* perform_search + handler response JSON (per_page clamp 1..100 else 20). */
int fg_db_search_json_ex(fg_db* db, const char* ns, const char* query, const char* const* filters,
                         uint32_t n_filters, uint32_t page, uint32_t per_page, int include_text, int shape, char* out,
                         size_t cap, size_t* len);
int fg_db_search_json(fg_db* db, const char* ns, const char* query, uint32_t page, uint32_t per_page,
                      int include_text, int shape, char* out, size_t cap, size_t* len);
/* POST /search/json (query_json_post, handlers/search.rs:210-301): the
 * JsonQueryRequest fields and the ?text= / ?include_data= URL flags, each flag
 * tri-state (-1 absent, 0 false, 1 true); has_page = 0 means no `page` object
 * (page 0, per_page 20).  Text: the URL flag wins, a disagreeing body flag adds
 * "developer_message"; "includes_data_objects" = body flag, else URL flag, else
 * not targeting; "targeting_conversations_or_organizations" = a filter
 * containing /conversation or /organization (handlers/utils.rs:4-14). */
int fg_db_search_json_post(fg_db* db, const char* ns, const char* query, const char* const* filters,
                           uint32_t n_filters, int has_page, uint32_t page, uint32_t per_page, int url_text,
                           int body_text, int url_include_data, int body_include_data, char* out, size_t cap,
                           size_t* len);
/* Stored facets of doc `doc` as Facet Display strings, '\n'-separated. */
int fg_db_doc_facets(fg_db* db, const char* ns, uint32_t doc, char* out, size_t cap, size_t* len);

/* ---- facet counts (src/db/facet.rs; fg_count_batch on the device).
 * Facets come back as Facet Display strings, '\n'-separated, in encoded-facet
 * byte order (FacetCounts::get's), with out_counts[i] the count of the i-th;
 * *n_out = how many.  Both *len and *n_out are set whenever the count ran, also
 * when a buffer is NULL or too small (out_paths: cap < *len + 1; out_counts:
 * count_cap < *n_out; either: FG_EINVAL), so one retry with the reported sizes fits.  A facet no matching doc
 * carries is not listed.  The namespace's current segments are counted under the
 * snapshot reference a search holds; nothing committed yet: no facets. */
/* list_facet / get_facets_at (:78-110), and the count the reference left
 * commented out (src/db/search.rs:436-454) over ALL matches: the direct children
 * of root_path ("/" = the top level) among the docs matching `query` (NULL or
 * blank: AllQuery; parsed as fg_db_search_ex parses it; a phrase or group
 * clause: FG_EUNSUPPORTED unless fg_count_clauses(1) is set) and `filters`;
 * *total (may be NULL) = the matching docs. */
int fg_db_facet_counts(fg_db* db, const char* ns, const char* query, const char* const* filters, uint32_t n_filters,
                       const char* root_path, char* out_paths, size_t cap, size_t* len, uint64_t* out_counts,
                       uint32_t count_cap, uint32_t* n_out, uint64_t* total);
/* get_facet_tree's collect_facets_recursive (:113-233) under "/": every facet
 * with its AllQuery count in pre-order, at most max_depth levels deep (< 0: no
 * limit; 0: nothing), from ONE device call instead of one collector pass per node. */
int fg_db_facet_tree(fg_db* db, const char* ns, int max_depth, char* out_paths, size_t cap, size_t* len,
                     uint64_t* out_counts, uint32_t count_cap, uint32_t* n_out);
/* GET /namespaces/{ns}/facets (handlers/namespaces.rs:45-87 over
 * DatasetManager::get_namespace_facets(ns, "/"), src/db/config.rs:251-255, which is
 * get_facets_at("/") on the namespace's dataset: the direct children of the root):
 * {"facets":[{"count":..,"path":..},..],"namespace":..,"status":"success"}. */
int fg_db_facets_json(fg_db* db, const char* ns, char* out, size_t cap, size_t* len);

/* Analyzer / parser exposed for tests: tokens separated by '\n'. */
int fg_analyze(const char* text, char* out, size_t cap, size_t* len);
/* mode (FG_MODE_AND / FG_MODE_OR: every clause Must / Should; FG_MODE_MIXED
 * otherwise) and the analyzed terms ('\n'-separated). */
#define FG_MODE_MIXED 2
int fg_parse_query(const char* query, int* mode, char* out, size_t cap, size_t* len);
/* The terms with their occurs: one line per term, "<o>:<term>", o = FG_OCCUR_*
 * ('0' Must, '1' Should, '2' MustNot). */
int fg_parse_query_occur(const char* query, char* out, size_t cap, size_t* len);
/* (Both return FG_EUNSUPPORTED for a query with a phrase clause: their outputs
 * cannot express one.)  The clauses, one line each: "<o>:" followed by the
 * clause's space-separated "term@pos" -- pos the token's position offset within
 * its phrase (a token the analyzer dropped leaves a hole); a term clause is a
 * single "term@0". */
int fg_parse_query_clauses(const char* query, char* out, size_t cap, size_t* len);
/* FacetTokenizer tokens of Facet::from_text(path), '\n'-separated; the
 * encoded facets keep their U+0000 separators, so read *len bytes. */
int fg_facet_tokens(const char* path, char* out, size_t cap, size_t* len);
/* build_facet_query's clause list for `filters` (encoded facet terms,
 * '\n'-separated, *len bytes); *applies = some filter survives the wildcard
 * split; *all_query = none parsed into a term (facet_query = AllQuery). */
int fg_facet_clauses(const char* const* filters, uint32_t n_filters, int* applies, int* all_query, char* out,
                     size_t cap, size_t* len);

#ifdef __cplusplus
}
#endif
#endif /* FUGU_HOST_H */
