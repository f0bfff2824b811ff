/*
 * omnirecall_hip.h -- C ABI of libomnirecall_hip.so, the MI355X (gfx950) scorer
 * behind the reference's IRecallSearchService seam.
 *
 * The reference has no FFI of its own: its only seam for this path is the DI
 * interface
 *     IRecallSearchService.SearchAsync(string query, int topK, CancellationToken)
 *         src/OmniRecall.Api/Services/RecallSearchService.cs:6-9   (registered Program.cs:59)
 * A drop-in GpuRecallSearchService keeps RecallSearchService.cs:22-25 (validate,
 * embed) and :39-56 (file names, snippet, Math.Round, DTO) in C#, and replaces
 * :26-37 -- GetRecentChunksAsync(300) + Select(ScoreChunk) + OrderByDescending /
 * ThenByDescending / Take -- with ONE call into this library.  INTEGRATION.md
 * shows the P/Invoke declarations that bind exactly these symbols.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++ / torch types, no exceptions.
 *   - every function returning int returns ORR_OK (0) or a negative orr_status;
 *     orr_last_error() gives the thread-local message.  Numeric guard cases of
 *     the reference (empty vector, dimension mismatch, zero norm;
 *     RecallSearchService.cs:71-72,84-85) are NOT errors: they score cosine 0.
 *   - the caller owns every buffer it passes; the library reads inputs only for
 *     the duration of the call (append copies) and owns device memory behind
 *     the opaque handle.  Strings cross as UTF-8 bytes with explicit offsets;
 *     nothing relies on NUL termination; nothing is freed across the ABI.
 *   - pointers marked "host or device" may be either; the library copies with
 *     hipMemcpyDefault.  The library works on its own non-blocking HIP streams: device-resident
 *     inputs must be COMPLETE (their producing stream synchronised, or an event waited for)
 *     before the call, and device-resident outputs are complete when the call returns.
 *   - threads: searches on a sealed index may be issued from any thread and run CONCURRENTLY on one
 *     handle (RecallSearchService is scoped per request, Program.cs:59; the store behind it is
 *     lock-free, InMemoryIngestionStore.cs:8-9): each takes a search lane of the index -- its own
 *     workspaces, or those of an internal view created on demand, up to the "max_lanes" option
 *     (default 4; corpus and shadows are shared, a lane costs its workspaces); further callers wait
 *     for a lane.  append / seal / delete / options wait until no search is in flight.
 */
#ifndef OMNIRECALL_HIP_H
#define OMNIRECALL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORR_ABI_VERSION 1

typedef enum orr_status {
    ORR_OK      = 0,
    ORR_EINVAL  = -1,   /* bad argument -> ArgumentException (RecallSearchService.cs:22-23)   */
    ORR_ENOMEM  = -2,   /* host or device allocation failed                                   */
    ORR_EDEVICE = -3,   /* HIP runtime / kernel failure, or no gfx950 device                   */
    ORR_ECOMM   = -4,   /* shard exchange inconsistent (merge input malformed)                 */
    ORR_EDIM    = -5,   /* appended embedding dimension differs from the index dimension       */
    ORR_ESTATE  = -6,   /* call not valid in this state (append after seal, search before)     */
    ORR_ELIMIT  = -7    /* the request is larger than a sticky limit allows (orr_search_range_cosine) */
} orr_status;

typedef struct orr_index orr_index;      /* opaque: one corpus shard resident on one GPU */

typedef struct orr_config {
    int32_t struct_size;      /* sizeof(orr_config), for forward compatibility                  */
    int32_t device;           /* HIP device ordinal                                             */
    int32_t dim;              /* embedding dimension D of every stored vector; 0 = corpus
                                 without embeddings (NoOpEmbeddingClient.cs:7): cosine is 0     */
    int32_t flags;            /* reserved, 0                                                    */
    int64_t capacity_rows;    /* rows to reserve up front; 0 = grow on demand                   */
    int64_t row_base;         /* position of this shard's first row in the GLOBAL
                                 CreatedAt-descending candidate order (0 on a single GPU)       */
} orr_config;

/* One ranked-candidate record as exchanged between shards (56 bytes).  A shard
 * emits kprime of these per query plus one trailer (see orr_search_shard). */
typedef struct orr_candidate {
    double  approx_score;   /* device-side fused score used for selection                      */
    double  dot;            /* sum_i (double)fl32(q_i * e_i), reference order (…cs:77-82)      */
    double  norm_b;         /* sum_i (double)fl32(e_i * e_i); 0 for rows without an embedding  */
    int64_t created_ticks;  /* CosmosChunkRecord.CreatedAtUtc.Ticks                            */
    int64_t row_id;         /* caller's id of the row (see orr_index_append); -1 = no record   */
    int64_t order_key;      /* global candidate position (row_base + position in the shard)    */
    int32_t matches;        /* query terms found in the content (…cs:111)                      */
    int32_t flags;          /* ORR_CAND_* bits                                                 */
    /* trailer record (index kprime of each query): approx_score = score of the
     * worst kept candidate, or -inf when the shard kept every participating row;
     * row_id = -1; order_key = rows that took part on this shard; matches =
     * number of valid records in front of it; flags = ORR_CAND_TRAILER.       */
} orr_candidate;

#define ORR_CAND_TRAILER   1
#define ORR_CAND_DOT_EXACT 2   /* `dot` is already the reference-order fp64 sum */
#define ORR_CAND_OVERFLOW  4   /* trailer only: the shard's candidate buffer overflowed; repeat unfused */
#define ORR_CAND_TWO_STAGE 8   /* trailer only: norm_b holds L; every row not offered has an exact score < L */
#define ORR_CAND_DEAD      16  /* the row was deleted (orr_index_delete_rows): the host finish drops the record */

/* Per-kernel timing collected with HIP events on the index's own stream. */
typedef struct orr_kernel_stat {
    char    name[48];
    int64_t launches;
    double  total_ms;        /* sum of hipEventElapsedTime over those launches                 */
    double  algo_bytes;      /* algorithmic bytes summed over those launches       */
} orr_kernel_stat;

/* Counters of one index since the last reset (orr_index_search_stats): how often the cheap passes had to be
 * repeated, and what the screening pass of the two-stage search kept.  128 bytes. */
typedef struct orr_search_stats {
    int64_t searches;            /* orr_search_batch calls                                                    */
    int64_t queries;             /* queries in them                                                           */
    int64_t passes;              /* device passes run for them (= searches when nothing had to be repeated)   */
    int64_t requeried;           /* queries that went through another pass (summed over repeats)              */
    int64_t overflowed_queries;  /* queries whose survivors did not fit their buffer in some pass             */
    int64_t buffer_growths;      /* times the survivors' buffers were enlarged from the measured counts       */
    int64_t exact_pass_queries;  /* queries that ended in the reference-arithmetic pass over every row        */
    int64_t survivors_total;     /* (query,row) pairs kept by the screening pass, summed over queries         */
    int64_t survivor_samples;    /* queries counted in survivors_total                                        */
    int64_t survivors_max;       /* largest count of one query                                                */
    int64_t survivor_capacity;   /* buffer entries per query the index uses now                               */
    int64_t vocab_tokens;        /* distinct whitespace-free tokens of the shard's contents (the keyword index)  */
    int64_t kw_hits_total;       /* (distinct query term, vocabulary token containing it) pairs, summed over passes */
    int64_t kw_passes;           /* passes that had query terms                                                */
    int64_t pass_mode;           /* what the LAST device pass ran: 0 no two-stage pass (exact kernel, unfused batched pass,
                                    large-k sort); 1 two-stage on the int8 shadow; 2 two-stage on the bf16 shadow; 3 two-stage
                                    WITHOUT a shadow (fp32 rows converted inside the kernel: "two_stage" = 2, or the shadow
                                    did not fit in device memory and "two_stage" = 1 fell back); 4 scoped pass
                                    (orr_search_batch_scoped: no screen, the listed rows re-scored exactly; also the list path
                                    of orr_search_batch_masked); 5 two-stage screen under a scope mask
                                    (orr_search_batch_masked); 6 two-stage screen under the masks of several groups at
                                    once (orr_search_batch_masked_groups; 4 or 5 where a group's own path ran last)        */
    int64_t reserved[1];         /* orr_cluster_search_stats: record exchanges done by RCCL all-gather ("exchange" = 1)      */
} orr_search_stats;

int         orr_abi_version(void);
int         orr_device_count(void);                 /* gfx950 devices visible; 0 if none        */
const char *orr_last_error(void);                   /* thread-local, never NULL                 */

/* ---- corpus shard -------------------------------------------------------
 * Replaces the data side of InMemoryIngestionStore.GetRecentChunksAsync
 * (InMemoryIngestionStore.cs:57-65): rows are CosmosChunkRecord projections
 * (Data/Models/CosmosIngestionRecords.cs:19-30). */
int  orr_index_create(const orr_config *cfg, orr_index **out);
void orr_index_destroy(orr_index *idx);

/* Appends n rows in the store's enumeration order (copies; host or device
 * pointers).
 *   dim            == cfg.dim with emb = [n][dim] row-major fp32, or 0 with
 *                  emb = NULL for rows whose Embedding is null/empty.  Any other
 *                  dim is ORR_EDIM (a mixed-dimension corpus is not supported;
 *                  in the reference such rows always score cosine 0 unless the
 *                  query has that same odd dimension).
 *   created_ticks  [n]    DateTime.Ticks of CreatedAtUtc.
 *   content_lower  UTF-8 of Content.ToLowerInvariant() (RecallSearchService.cs:110
 *                  is hoisted to ingest; the C# shim calls ToLowerInvariant itself).
 *   content_off    [n+1]  byte offsets into content_lower.
 *   row_ids        [n] ids returned by searches, or NULL for
 *                  row_base + (rows appended so far) + i.                        */
int orr_index_append(orr_index *idx, int64_t n, int32_t dim, const float *emb,
                     const int64_t *created_ticks, const uint8_t *content_lower,
                     const uint64_t *content_off, const int64_t *row_ids);

/* Puts rows into candidate order -- stable CreatedAt-descending, i.e. what
 * OrderByDescending(c => c.CreatedAtUtc) yields (InMemoryIngestionStore.cs:61) --
 * and precomputes the exact row norms.  Required before searching. */
int     orr_index_seal(orr_index *idx);
/* Moves the shard within the global candidate order (a newer shard was put in front of it):
 * only order keys and the clipping of candidate_limit depend on it. */
int     orr_index_set_row_base(orr_index *idx, int64_t row_base);
int64_t orr_index_rows(const orr_index *idx);
int32_t orr_index_dim(const orr_index *idx);

/* ---- search -------------------------------------------------------------
 * One batch of B queries against a sealed single-GPU index; replaces
 * RecallSearchService.cs:26-37 for each query.
 *   dim, q          query vectors [B][dim] (host or device); dim 0 = empty
 *                   vector (EmbeddingResult.Vector = []), q may be NULL.
 *   terms_utf8, term_off, query_term_off
 *                   the queryTerms of RecallSearchService.cs:95-108, already split,
 *                   lowercased, de-duplicated and stop-word filtered by the host:
 *                   term t is terms_utf8[term_off[t] .. term_off[t+1]); query b owns
 *                   terms query_term_off[b] .. query_term_off[b+1).  A query with no
 *                   terms has keyword score 0 (:100-101).
 *                   These three arrays are HOST memory.
 *   now_ticks       the frozen DateTime.UtcNow.Ticks for :117.
 *   topk            Take(Math.Max(1, topK)) (:36).
 *   candidate_limit GetRecentChunksAsync(maxCount) (:26): 300 reproduces the
 *                   reference, >= rows scores the whole corpus.
 *   out_rows, out_scores  [B][max(1,topk)]: row ids and UNROUNDED fused scores in
 *                   rank order (score desc, CreatedAt desc, candidate order).
 *   out_counts      [B]: citations actually produced (< topk on a small corpus). */
int orr_search_batch(orr_index *idx, int32_t B, int32_t dim, const float *q,
                     const uint8_t *terms_utf8, const uint32_t *term_off,
                     const uint32_t *query_term_off, int64_t now_ticks, int32_t topk,
                     int64_t candidate_limit, int64_t *out_rows, double *out_scores,
                     int32_t *out_counts);

/* Row-sharded corpus, step 1 (runs on every shard's GPU): the shard's best
 * kprime candidates per query, selected on (score desc, global candidate
 * position asc).  out: [B][kprime+1] records (host or device), the last one of
 * each query being the trailer.  candidate_limit is GLOBAL; the shard clips it
 * with its row_base. */
int orr_search_shard(orr_index *idx, int32_t B, int32_t dim, const float *q,
                     const uint8_t *terms_utf8, const uint32_t *term_off,
                     const uint32_t *query_term_off, int64_t now_ticks, int32_t kprime,
                     int64_t candidate_limit, orr_candidate *out);

/* The same with the two per-call choices as ARGUMENTS instead of sticky index options ("shard_topk", "shard_pass", which
 * orr_search_shard reads): topk = the caller's k when > 0 (the two-stage floor then comes from the k-th best score of the
 * sampled prefix, not the k'-th: fewer survivors; valid across shards, the global k-th best is at least every shard's);
 * pass = 0 the library's choice, 1 the unfused batched pass, 2 the reference-arithmetic pass over every row (the repeat of
 * queries orr_merge_candidates could not certify).  Passes 1 and 2 keep one number per (query,row): they run over slices
 * of the batch so that their workspace stays below 4 GiB whatever B. */
int orr_search_shard_ex(orr_index *idx, int32_t B, int32_t dim, const float *q,
                        const uint8_t *terms_utf8, const uint32_t *term_off,
                        const uint32_t *query_term_off, int64_t now_ticks, int32_t kprime,
                        int64_t candidate_limit, int32_t topk, int32_t pass, orr_candidate *out);

/* Row-sharded corpus, step 2 (host only, no GPU needed): merges the gathered
 * records of n_shards shards ([n_shards][B][kprime+1], host memory), rescoring
 * every candidate in the reference's exact arithmetic and ranking with the exact
 * key.  index_dim is the shards' embedding dimension (cosine applies only when
 * dim == index_dim > 0, RecallSearchService.cs:71).  *out_uncertified (may be NULL) receives the number of queries whose
 * top-k could not be certified against the shards' cut-off scores -- the caller
 * should repeat both steps with a larger kprime for those. */
int orr_merge_candidates(int32_t n_shards, int32_t B, int32_t kprime, const orr_candidate *all,
                         int32_t index_dim, int32_t dim, const float *q_host,
                         const uint32_t *query_term_off, int64_t now_ticks, int32_t topk,
                         int64_t *out_rows, double *out_scores, int32_t *out_counts,
                         int32_t *out_uncertified);

/* The same, also telling WHICH queries were certified: out_certified[B] (may be NULL), 1 = the query's top-k is final.  The
 * caller repeats only the others (as a compacted sub-batch, through orr_search_shard_ex with pass = 2, then a larger kprime):
 * every rank of a multi-process job holds identical gathered bytes, so all ranks pick the same sub-batch without a collective. */
int orr_merge_candidates_ex(int32_t n_shards, int32_t B, int32_t kprime, const orr_candidate *all,
                            int32_t index_dim, int32_t dim, const float *q_host,
                            const uint32_t *query_term_off, int64_t now_ticks, int32_t topk,
                            int64_t *out_rows, double *out_scores, int32_t *out_counts,
                            int32_t *out_uncertified, uint8_t *out_certified);

/* ---- shard file ---------------------------------------------
 * A sealed shard as one binary file (embeddings, exact norms, timestamps, row ids and the
 * token index), so that a corpus does not have to be re-ingested and re-sealed per run.
 * The reference's only durable form is Cosmos JSON (CosmosIngestionRecords.cs:19-30).
 * load: cfg->device and cfg->row_base are taken from cfg; dim comes from the file
 * (cfg->dim must be 0 or equal).  The loaded index is sealed. */
int orr_index_save(orr_index *idx, const char *path);
int orr_index_load(const orr_config *cfg, const char *path, orr_index **out);

/* ---- a second search lane ---------------------------------------------------
 * orr_index_view: another handle over the same SEALED shard with its own streams and workspaces.  It
 * borrows the corpus (and the bf16 shadow, built first if the two-stage pass is on): nothing is copied.
 * Searches on the index and on its views may run concurrently from different threads, which lets the
 * keyword chain, the ranking pass and the host finish of one batch overlap the screening pass of another
 * (the request path of Program.cs:59 is concurrent by nature).  A view must be destroyed before its
 * parent; it cannot be appended to, sealed again or saved. */
int orr_index_view(orr_index *parent, orr_index **view);

/* ---- deletes without a reseal -------------------------------------------------
 * Replaces InMemoryIngestionStore.DeleteDocumentAsync (InMemoryIngestionStore.cs:50-55) and the
 * "replace the chunk list" half of UpsertChunksAsync (:17-25) on a SEALED shard: the rows with the given
 * ids (the ids of orr_index_append) stop taking part in every later search, exactly as if the shard had
 * been rebuilt without them -- they are not ranked, and they do not count towards candidate_limit.  The
 * rows keep their positions (order_key of the others is unchanged, so is every row id), nothing is moved
 * in HBM: the cost is one small upload.  On the device a deleted row's norm and timestamp are overwritten
 * (its score drops to the keyword part, <= 0.2), its records are flagged ORR_CAND_DEAD and the host finish
 * (orr_search_batch, orr_merge_candidates) drops them; the certificate logic is unchanged, so results stay
 * exact.  Unknown and already deleted ids are skipped; *out_deleted (may be NULL) = rows newly deleted.
 * Exclusive like append/seal: no search may be in flight on the index or its views.  Views see the
 * deletes of their parent.  ORR_ESTATE once more than a quarter of the shard is deleted: rebuild it.
 * orr_index_live_rows = rows - deleted rows.  A shard behind others in the global order is told how many
 * deleted rows lie in front of it with the "dead_rows_before" option, so that candidate_limit keeps
 * counting live rows only.  orr_index_save / orr_index_load keep the deleted set. */
int     orr_index_delete_rows(orr_index *idx, int64_t n, const int64_t *row_ids, int64_t *out_deleted);
int64_t orr_index_live_rows(const orr_index *idx);

/* ---- reindex in place ----------------------------------------------------------
 * Replaces the vectors of sealed rows in place (reindex, DocumentIngestionService.cs:210-291): the reference
 * re-embeds every chunk of a document and upserts the list again with the same chunk ids, contents and
 * CreatedAtUtc (:277), so only the vectors change.  row_ids[n] are the ids of orr_index_append (host or device
 * memory); emb is [n][dim] fp32 (host or device memory).  dim == the index dimension: each row gets its new
 * vector; dim 0 with emb NULL: the rows lose their embedding (zero rows with norm 0, as orr_index_append stores a
 * row without one); any other dim is ORR_EDIM, and an index created with dim 0 is ORR_ESTATE.  Afterwards the
 * shard holds the same bytes a shard sealed from scratch with the new vectors would hold: embeddings, exact norms,
 * and the rows of the int8 and bf16 shadows where those exist (shadows not built yet are built later from the new
 * rows).  The token index, timestamps, row ids and candidate order stay as they are, nothing moves in HBM, so
 * internal lanes and views (orr_index_view) see the new rows at once; views do not block the call.  Unknown and
 * deleted ids are skipped (writing a deleted row would bring it back); every live row carrying a listed id is
 * updated (duplicate ids of orr_index_append); an id listed twice is ORR_EINVAL before anything is written.
 * *out_updated (may be NULL) = rows written.  Needs a sealed index (ORR_ESTATE) and the owning handle (ORR_EINVAL
 * on a view).  Exclusive like delete: waits for the searches in flight.  The input goes through a device staging
 * buffer of at most 256 MiB of rows per round: no second copy of the shard.  Cost: about 2 x 4 x dim bytes of
 * HBM traffic per row plus the upload.  ORR_EDEVICE part way through leaves the listed rows in an unspecified mix
 * of old and new: rebuild the shard. */
int     orr_index_update_rows(orr_index *idx, int64_t n, const int64_t *row_ids, int32_t dim, const float *emb,
                              int64_t *out_updated);

/* ---- compaction ------------------------------------------------------------------
 * Rebuilds a sealed shard IN PLACE without its deleted rows -- the other half of "replace the chunk list"
 * (InMemoryIngestionStore.cs:17-25, 50-55), where the reference simply drops the old list: embeddings move up
 * chunk by chunk through a 256 MiB bounce buffer (no second copy of the shard), norms / timestamps / ids are
 * gathered, every posting list of the token index loses the deleted positions and is renumbered, the shadows are
 * dropped and rebuilt at the next search that wants them.  Row ids are kept; positions (order keys) close up, so a
 * shard BEHIND this one in a global order moves up by *out_removed (may be NULL) rows: give it its new row_base
 * (orr_index_set_row_base) and "dead_rows_before" -- orr_cluster_compact does both for a cluster.  Lifts the
 * quarter-of-the-shard limit of orr_index_delete_rows.  Exclusive like delete; ORR_ESTATE while views made with
 * orr_index_view are alive (they borrow the arrays that move).  A failure half way (ORR_EDEVICE / ORR_ENOMEM)
 * leaves the shard unusable: rebuild it. */
int orr_index_compact(orr_index *idx, int64_t *out_removed);

/* ---- rows into a sealed shard ------------------------------------------------------
 * The missing half of UpsertChunksAsync (InMemoryIngestionStore.cs:17-25) on a SEALED shard: an upsert takes any CreatedAtUtc,
 * and orr_index_append after the seal is ORR_ESTATE.  Arguments as orr_index_append (host or device pointers), except that
 * row_ids is REQUIRED (ORR_EINVAL when NULL): the default id of append, row_base + position, is no longer unique once a shard
 * was compacted.  Afterwards the shard is what a shard sealed from scratch from (the old rows in candidate order, then these
 * rows in the order given) would be -- a stable CreatedAt-descending merge: at equal ticks every old row stays in front of
 * every new one, new rows keep their relative order.  Embeddings bit for bit, exact norms (of the new rows: taken on the
 * staging buffer by the kernel the seal uses), timestamps, row ids, and the token index as a map token -> ascending positions
 * (tokens not seen before are appended to the vocabulary, so its ORDER, and with it the bytes of a shard file, may differ from
 * a fresh seal's; searches do not).  Deleted rows stay deleted at their shifted positions.  orr_index_rows grows by n and rows
 * behind an insertion point move down: a shard BEHIND this one in a global order moves down by n rows -- give it its new
 * row_base (orr_index_set_row_base); orr_cluster_insert_rows does that for a cluster.  *out_inserted (may be NULL) = n.
 *   dim   == the index dimension with emb = [n][dim], or 0 with emb = NULL for rows without an embedding (zero rows, norm 0);
 *         any other dim is ORR_EDIM.  n == 0: ORR_OK, nothing is touched.  rows + n >= 2^32 - 1: ORR_EINVAL.
 * Needs a sealed index (ORR_ESTATE) and the owning handle (ORR_EINVAL on a view); ORR_ESTATE while views made with
 * orr_index_view are alive (they borrow the arrays that move).  Exclusive like compact: waits for the searches in flight;
 * internal lanes are remade on demand.  A shadow (int8, bf16) that was built before the call is rebuilt from the moved rows
 * before the call returns, one that was not stays unbuilt; token bitmaps are rebuilt at the next search that wants them.
 * A shadow that cannot be rebuilt (no room for the grown shard, or a failure inside its build) is dropped and the call still
 * returns ORR_OK: the rows are in, and the next search that wants the shadow builds it as on a new shard.
 * Memory: with room reserved (orr_config.capacity_rows, or what the 1.5 x growth of append left) the embeddings move IN
 * PLACE, from the last destination chunk to the first, through a bounce buffer of at most 256 MiB; the new rows come
 * through a staging buffer of at most 256 MiB per round; rows in front of the first insertion point are not touched.
 * WITHOUT room (a shard from orr_index_load has exactly its rows) the arrays are grown first, which takes a second copy of
 * the embeddings for the duration of the copy, or ORR_ENOMEM.  Every allocation happens before the first row moves:
 * ORR_ENOMEM leaves the shard exactly as it was and searchable.  ORR_EDEVICE part way leaves it unusable: rebuild it. */
int orr_index_insert_rows(orr_index *idx, int64_t n, int32_t dim, const float *emb,
                          const int64_t *created_ticks, const uint8_t *content_lower,
                          const uint64_t *content_off, const int64_t *row_ids, int64_t *out_inserted);

/* ---- scoped search: rank only the rows a caller lists ---------------------------------------
 * "Search inside these documents" (IIngestionStore.GetChunksByDocumentIdAsync, IIngestionStore.cs:11, and the per-document
 * endpoints), or inside whatever a host's own metadata filter selected.  Query b's scope S_b is a multiset of row ids (the ids
 * of orr_index_append): scope_ids[scope_off[b] .. scope_off[b+1]); scope_off == NULL: all B queries share the whole list.
 * scope_ids is host or device memory, scope_off[B+1] host memory.
 *   result      what orr_search_batch would return on a shard sealed from scratch from only the LIVE rows whose id is in S_b, in
 *               their present candidate order, arguments otherwise the same: rows, order and fp64 scores bit for bit.
 *   ids         unknown ids and ids of deleted rows are skipped; an id listed twice counts once; an id carried by several
 *               rows (duplicate ids at append) brings every live one of them, as in orr_index_update_rows.
 *   candidate_limit  counts scoped live rows only: the first max(1, candidate_limit) of them in candidate order take part
 *               (GetRecentChunksAsync(maxCount) over a store that holds only those chunks).
 *   empty       an empty scope, or one without a live row, gives out_counts[b] = 0.
 * topk, dim 0 / another dimension, rows without an embedding, NaN order and ties: as orr_search_batch.
 * A scoped search is a search: it takes a lane, runs beside other searches, works on views, counts in orr_search_stats
 * (pass_mode 4).  It never builds a shadow and never runs a pass over all rows: the listed ids are resolved on the device
 * through a table of the shard's (id, position) pairs sorted by id -- 12 bytes per row, built at the first scoped search
 * (ORR_ENOMEM when it does not fit), shared by the lanes and views, dropped by orr_index_insert_rows and orr_index_compact,
 * never saved -- and the exact re-score of the two-stage pass reads the listed rows only: about 4 x dim bytes of HBM per
 * (query, scoped row) pair.  Large scopes shared by many queries are therefore the wrong tool.
 * "Never builds a shadow" is about the search itself: a concurrent search that makes another lane of the handle goes through
 * orr_index_view's preparation, which builds the shadow of a two-stage-sized shard with "two_stage" = 1 as for any search.
 * One query may bring at most 4,194,240 scoped rows (after the candidate_limit clip) to a search: ORR_EINVAL beyond that.
 * Argument errors (ORR_EINVAL before any device call): a null index, n_scope_ids < 0, scope_ids NULL with n_scope_ids > 0,
 * offsets that do not start at 0, decrease, or do not end at n_scope_ids. */
int orr_search_batch_scoped(orr_index *idx, int32_t B, int32_t dim, const float *q,
                            const uint8_t *terms_utf8, const uint32_t *term_off, const uint32_t *query_term_off,
                            int64_t now_ticks, int32_t topk, int64_t candidate_limit,
                            int64_t n_scope_ids, const int64_t *scope_ids, const uint64_t *scope_off,
                            int64_t *out_rows, double *out_scores, int32_t *out_counts);

/* Row-sharded form, with the record contract of orr_search_shard: [B][kprime+1] records (host or device), every record with
 * ORR_CAND_DOT_EXACT, the trailer's order_key = the scoped rows that took part on this shard and approx_score = -inf when all
 * of them are records: orr_merge_candidates(_ex) is used unchanged.  topk as orr_search_shard_ex (0: unknown).
 * candidate_limit is GLOBAL over scoped live rows: the shard lets its first max(0, candidate_limit - scope_before[b]) take
 * part, scope_before[b] (host memory; NULL: zeros) being query b's scoped live rows on the shards in front of this one
 * (orr_index_scope_count).  row_base only enters order_key. */
int orr_search_shard_scoped(orr_index *idx, int32_t B, int32_t dim, const float *q,
                            const uint8_t *terms_utf8, const uint32_t *term_off, const uint32_t *query_term_off,
                            int64_t now_ticks, int32_t kprime, int64_t candidate_limit, int32_t topk,
                            int64_t n_scope_ids, const int64_t *scope_ids, const uint64_t *scope_off,
                            const int64_t *scope_before, orr_candidate *out);

/* ---- masked search: one scope shared by every query of the batch, screened once per batch ----
 * A tenant's rows, a collection, a time window: a LARGE scope that the whole batch shares.  scope_ids[0 .. n_scope_ids) (host
 * or device memory) is that scope.  The result is exactly what orr_search_batch_scoped defines for scope_off == NULL -- what
 * orr_search_batch would return on a shard sealed from scratch from only the live rows whose id is listed, in their present
 * candidate order: rows, order and fp64 scores bit for bit -- and ids (unknown, deleted, listed twice, carried by several
 * rows), candidate_limit (counts scoped live rows), an empty scope (counts of 0), topk, dim 0 or another dimension, NaN order,
 * ties and the argument errors are as documented there.
 * What differs is the cost.  The scoped call re-scores every listed row once per query; this call streams the shard's shadow
 * ONCE per batch through the two-stage screen with the scope as a mask on the rows (pass_mode 5), re-scores an in-scope
 * sample of about sqrt(topk x scoped rows) rows per query for the floor, and re-scores the survivors exactly.  Unlike the
 * scoped call it therefore MAY build a shadow ("two_stage") and MAY run a pass over all rows of the shard in front of the
 * scope's last row.  Where the screen does not apply (what a two-stage pass needs: a cosine part, dim % 64 == 0,
 * max(1, topk) <= 64, at least 196,608 rows in front of the scope's last row, "two_stage" != 0; and a scope larger than the
 * sample) or does not pay ("mask_screen"), and for queries the screen cannot certify, the call runs the scoped pass over the
 * scope in parts of at most "mask_part_rows" rows (pass_mode 4).  There is NO limit on the size of the scope: this call never
 * answers ORR_EINVAL for a scope that is too large.
 * A masked search is a search: it takes a lane, runs beside other searches, works on views, counts in orr_search_stats
 * (survivors_* count what is left behind the mask; exact_pass_queries is never raised), and uses the id table of the scoped
 * search (12 bytes per row, built at the first scoped or masked search). */
int orr_search_batch_masked(orr_index *idx, int32_t B, int32_t dim, const float *q,
                            const uint8_t *terms_utf8, const uint32_t *term_off, const uint32_t *query_term_off,
                            int64_t now_ticks, int32_t topk, int64_t candidate_limit,
                            int64_t n_scope_ids, const int64_t *scope_ids,
                            int64_t *out_rows, double *out_scores, int32_t *out_counts);

/* Row-sharded form of the masked search, with the record contract of orr_search_shard / orr_search_shard_scoped: [B][kprime+1]
 * records (host or device `out`), the last record of each query its trailer; orr_merge_candidates(_ex) is used unchanged.
 *   scope            ONE list shared by the batch (host or device memory), resolved as orr_search_batch_masked resolves it (id
 *                    table, one bitmap, deleted rows left out; unknown ids, ids listed twice and ids carried by several rows as
 *                    documented there).
 *   candidate_limit  GLOBAL over scoped live rows: the shard lets its first took = min(live, max(0, max(1, candidate_limit) -
 *                    scope_before)) scoped live rows take part, scope_before being the scope's live rows on the shards in front
 *                    of this one (orr_index_scope_count there; ONE number, the scope is shared).  row_base only enters
 *                    order_key.
 *   kprime           ONE pass at the caller's kprime, no ladder inside: the caller's merge certifies.  Only the queries whose
 *                    survivors' buffers overflowed repeat once inside the call with buffers sized from the measured counts;
 *                    after that the trailer carries ORR_CAND_OVERFLOW.
 *   pass             0: the library's choice -- the masked screen where it is eligible and pays for this shard's took rows in
 *                    front of this shard's clip ("mask_screen"), else the list path; 1: the list path in parts
 *                    ("mask_part_rows"), never the screen.  A kprime above a selection list (64), or a batch no two-stage form
 *                    exists for, takes the list path whatever `pass` says (beyond a list: every scoped row scored, reduced to
 *                    kprime records on the host).
 *   topk             as orr_search_shard_ex (0: unknown): the floor comes from the min(kprime, topk)-th best of the shard's
 *                    in-scope sample -- valid across shards, the global k-th best is at least every shard's.
 *   trailer          order_key = took, matches = the valid records.  Behind the screen ORR_CAND_TWO_STAGE with the floor L in
 *                    norm_b (every scoped row not offered scores below L); behind the list path no floor, and every record has
 *                    ORR_CAND_DOT_EXACT.  took == 0 (an empty shard, an empty list, a limit used up in front): empty records
 *                    and a trailer that cut nothing.
 * It is a search: it takes a lane, runs beside other searches, works on views and counts in orr_search_stats (pass_mode 5 or 4).
 * ORR_EINVAL before any device call: the masked call's argument errors, kprime < 1, topk < 0, pass outside {0, 1},
 * scope_before < 0, out NULL. */
int orr_search_shard_masked(orr_index *idx, int32_t B, int32_t dim, const float *q,
                            const uint8_t *terms_utf8, const uint32_t *term_off, const uint32_t *query_term_off,
                            int64_t now_ticks, int32_t kprime, int64_t candidate_limit, int32_t topk, int32_t pass,
                            int64_t n_scope_ids, const int64_t *scope_ids, int64_t scope_before, orr_candidate *out);

/* ---- grouped masked search: several large scopes share one screening pass ----
 * Requests that arrive together belong to different tenants, collections or time windows: G scopes, each shared by the queries
 * that name it.  Group g's ids are scope_ids[group_off[g] .. group_off[g + 1]) (scope_ids host or device memory; group_off
 * host memory, n_groups + 1 entries); query b searches inside group query_group[b] (host memory, B entries).
 * Query b's result is exactly what orr_search_batch_masked returns for that query with group query_group[b]'s ids as the
 * scope -- what orr_search_batch would return on a shard sealed from only the live rows of that group: rows, order and fp64
 * scores bit for bit.  candidate_limit counts each group's own scoped live rows; ids (unknown, deleted, listed twice, carried
 * by several rows), an empty group (counts of 0), topk, dim, NaN order and ties are as documented for the masked call.  Groups
 * may overlap, may be equal, may be empty, and may be named by no query.
 * What differs is the cost.  A masked call per group streams the shard's shadow once per GROUP; this call streams it once per
 * BATCH: the groups large enough to screen (more rows than their in-scope sample) run through ONE two-stage pass whose row
 * constants admit every such group's rows, whose floor comes per query from a sample of its own group, and whose survivors are
 * filtered per query against its own group's bitmap and clip (pass_mode 6).  Smaller groups, groups of a batch in which the
 * grouped pass is not eligible or does not pay ("mask_screen": 0 by the summed cost rule -- the sum over the screening groups
 * of max(max(4 x queries of the group, 128) x scoped rows, 524,288) >= rows in front of the last group's last row --, 1
 * whenever eligible, 2 never), and queries the grouped pass cannot certify run as a masked call of their group (pass_mode 5
 * or 4).  One used group (named by a query, with a live row) IS the masked call.  A buffer growth of the grouped pass is the
 * call's own: it counts in buffer_growths and leaves survivor_capacity alone.
 * ORR_EINVAL before any device call, with the outputs untouched: the masked call's argument errors, n_groups outside 1 .. 64
 * (a stated cap: the group bitmaps take n_groups x rows / 8 bytes), group_off or query_group NULL, offsets that do not start at
 * 0, decrease, or do not end at n_scope_ids, a query_group[b] outside [0, n_groups).
 * The call is a search: it takes a lane, runs beside other searches, works on views and counts in orr_search_stats. */
int orr_search_batch_masked_groups(orr_index *idx, int32_t B, int32_t dim, const float *q,
                                   const uint8_t *terms_utf8, const uint32_t *term_off, const uint32_t *query_term_off,
                                   int64_t now_ticks, int32_t topk, int64_t candidate_limit,
                                   int32_t n_groups, int64_t n_scope_ids, const int64_t *scope_ids,
                                   const uint64_t *group_off /* host [n_groups + 1] */,
                                   const int32_t *query_group /* host [B] */,
                                   int64_t *out_rows, double *out_scores, int32_t *out_counts);

/* out_live[B] (host memory): the live rows query b's scope resolves to on this shard. */
int orr_index_scope_count(orr_index *idx, int32_t B, int64_t n_scope_ids, const int64_t *scope_ids,
                          const uint64_t *scope_off, int64_t *out_live);

/* ---- scope handles: resolve a scope once, keep it through maintenance --------
 * The scoped, masked and grouped calls above take their scope as a list of row ids and resolve it on every call.  An orr_scope
 * is that resolve kept: a set of ROWS of one sealed shard, resident on its device as the bitmap the masked call builds, with
 * its counts.  It is fixed when the rows are added and follows those rows wherever maintenance moves them:
 *   orr_index_delete_rows      the deleted rows leave every scope
 *   orr_index_compact          positions close up; every scope is carried along (it holds no deleted row, so nothing leaves)
 *   orr_index_insert_rows      old rows move; every scope is carried along.  Rows inserted later belong to NO scope -- a time
 *                              window whose interval covers them included -- until orr_scope_add_ids names them; that call
 *                              looks up only the ids it is given and ORs them in.  A term scope is no exception: rows
 *                              inserted later are not in it even when their text contains its terms (it is not evaluated
 *                              again); an orr_scope_create_terms made afterwards holds them.  Nor is a cosine scope:
 *                              rows inserted later are not in it however close they lie to its probes, and
 *                              orr_index_update_rows does not evaluate it again either -- a row it held stays in it with its
 *                              new vector; an orr_scope_create_near made afterwards sees the rows as they are then
 *   orr_index_update_rows, orr_index_set_row_base   touch no scope
 * Unlike a view, a scope does not block compaction or insertion.  Scopes are not saved by orr_index_save.  A scope costs one
 * bit per row of the shard plus its chunk counts (1.25 MB at 10M rows); ORR_ENOMEM when that does not fit.
 *   orr_scope_create        resolves ids exactly as orr_search_batch_masked resolves its list: unknown ids and deleted rows are
 *                           passed over, an id listed twice counts once, an id carried by several rows brings all of them.
 *                           n_ids == 0 gives an empty scope.  ids may be host or device memory.
 *   orr_scope_create_ticks  the live rows with ticks_from <= CreatedAtUtc.Ticks < ticks_to.  Half-open, so adjacent windows
 *                           tile; ticks_from >= ticks_to gives an empty scope, not an error; INT64_MIN and INT64_MAX are the
 *                           open ends.  Rows are in CreatedAt-descending order, so this costs two binary searches on the host
 *                           and one fill, however large the window.
 *   orr_scope_create_terms  the live rows whose lowercased content contains EVERY term (ORR_TERMS_ALL) or AT LEAST ONE term
 *                           (ORR_TERMS_ANY) as a substring: the rows for which the keyword side of a search with these terms
 *                           would count n of n matches, or at least one (contentLower.Contains(term, Ordinal)).  The terms are
 *                           HOST memory in the form of orr_search_batch's: term t is terms_utf8[term_off[t] .. term_off[t+1]),
 *                           already lowercased, without whitespace; stop words are the caller's choice, a scope takes the
 *                           terms it is given.  A row without content is never in; a term that matches nothing empties ALL
 *                           and adds nothing to ANY; a term listed twice counts once.  n_terms == 0 gives an empty scope in
 *                           both modes, as n_ids == 0 does -- the scope of ALL live rows is
 *                           orr_scope_create_ticks(INT64_MIN, INT64_MAX), which is also the left side of "contains none of":
 *                           all rows ANDNOT the ANY scope.  At most 256 terms (a row bitmap of workspace per distinct term:
 *                           320 MB at 10M rows).  The keyword chain of a search runs once for the call, on the device; no
 *                           search statistic moves.
 *   orr_scope_create_near   the live rows r with CosineSimilarity(probe_p, e_r) >= min_cosine for EVERY probe (ORR_NEAR_ALL) or
 *                           for AT LEAST ONE (ORR_NEAR_ANY): the reference's function (RecallSearchService.cs:69-88) bit for
 *                           bit, compared as C# compares doubles.  probes is [n_probes][dim] floats in host or device memory.
 *                           The reference's guards stand: a row without an embedding has cosine 0, so has a probe or a row
 *                           with norm <= 0; dim 0 (probes may be NULL) or a dim other than the index's gives cosine 0 for
 *                           every row -- the scope is then every live row when 0 >= min_cosine and empty otherwise, and no row
 *                           is read; a NaN cosine is never >= anything.  min_cosine may be -infinity or +infinity.  A probe
 *                           listed twice counts once; n_probes == 0 gives the empty scope in both modes.  AT MOST 8 PROBES per
 *                           call (one walk of the rows carries 8): fold more with orr_scope_combine (AND for ALL, OR for ANY).
 *                           A set without a size limit, not a ranking: "everything but the rows close to X" is all rows
 *                           (orr_scope_create_ticks(INT64_MIN, INT64_MAX)) ANDNOT this scope.  The rows are walked once, in
 *                           the exact arithmetic of the search's exact pass; a pair whose cosine lies within 2^-40 of
 *                           min_cosine (or is not finite) is decided on the host by the expression the host finish of a search
 *                           uses.  Those pairs go through a list of "near_band_cap" entries of 16 bytes (orr_index_set_option,
 *                           default 65,536, 1 .. 2^31): a walk that needs more -- thousands of copies of the probe with
 *                           min_cosine at their own cosine -- grows the list to what it needed and runs once more.  No search
 *                           statistic moves.
 *   orr_scope_add_ids       adds the live rows that carry the ids; *out_added (may be NULL) = rows that were not in it before
 *   orr_scope_combine       dst = dst AND src, dst OR src, or dst AND NOT src, in place; src is unchanged (src == dst is allowed)
 *   orr_scope_rows          live rows in it now; -1 on an orphaned handle (or NULL)
 *   orr_scope_row_ids       the ids of its live rows in candidate order into out_ids (host memory, room for cap ids); *out_n =
 *                           their number.  Nothing is written beyond cap; ORR_EINVAL, after *out_n is set, when cap is too small
 *   orr_scope_destroy       frees it (NULL is allowed)
 * idx may be the owning index or any view of it.  A scope belongs to the shard it was made on: using it with another shard, or
 * combining scopes of two shards, is ORR_EINVAL.  orr_index_destroy of the owning index frees the device memory of the scopes
 * that are still alive and orphans them: every later call on one is ORR_ESTATE, orr_scope_rows is -1, and orr_scope_destroy
 * still has to be called to free the host part.  orr_scope_destroy and orr_index_destroy may be called from different threads
 * at the same time (the library serialises the two); a search, add_ids or combine on a scope must have returned before its
 * index is destroyed, as for every other call on that index.
 * If a delete, a compaction or an insertion has changed the rows but a device error then keeps the library from bringing a
 * scope's counts up to date, the call returns that error, the shard itself is whole, and that scope is orphaned (ORR_ESTATE
 * from then on) rather than searched with stale counts: make it again.
 * Threads: searches hold a scope shared, so any number may search one scope at once; add_ids, combine (on dst) and destroy hold
 * it exclusively and wait for them.  create, add_ids, combine and row_ids take a lane like a search.
 * ORR_EINVAL before any device call, with the outputs untouched, and before the index handle is looked at: a NULL scope or out
 * pointer, negative counts, ids NULL with n_ids > 0, op outside 0 .. 2; for orr_scope_create_terms, in this order: out NULL,
 * n_terms outside 0 .. 256, terms_utf8 or term_off NULL with n_terms > 0, mode outside 0 .. 1, an empty term or offsets that
 * decrease; for orr_scope_create_near, in this order: out NULL, n_probes outside 0 .. 8, dim negative, probes NULL with
 * n_probes > 0 and dim > 0, mode outside 0 .. 1, min_cosine NaN -- then a NULL index, then ORR_ESTATE for an index that is not
 * sealed. */
typedef struct orr_scope orr_scope;      /* opaque: a set of rows of one sealed shard, resident on its device */
#define ORR_SCOPE_AND    0
#define ORR_SCOPE_OR     1
#define ORR_SCOPE_ANDNOT 2
#define ORR_TERMS_ALL 0
#define ORR_TERMS_ANY 1
#define ORR_NEAR_ALL 0
#define ORR_NEAR_ANY 1
int     orr_scope_create(orr_index *idx, int64_t n_ids, const int64_t *ids /* host or device */, orr_scope **out);
int     orr_scope_create_ticks(orr_index *idx, int64_t ticks_from, int64_t ticks_to, orr_scope **out);
int     orr_scope_create_terms(orr_index *idx, int32_t n_terms, const uint8_t *terms_utf8 /* host */, const uint32_t *term_off /* host [n_terms+1] */,
                               int32_t mode, orr_scope **out);
int     orr_scope_create_near(orr_index *idx, int32_t n_probes, int32_t dim, const float *probes /* host or device, [n_probes][dim] */,
                              double min_cosine, int32_t mode, orr_scope **out);
int     orr_scope_add_ids(orr_scope *s, int64_t n_ids, const int64_t *ids /* host or device */, int64_t *out_added);
int     orr_scope_combine(orr_scope *dst, int32_t op, const orr_scope *src);
int64_t orr_scope_rows(const orr_scope *s);
int     orr_scope_row_ids(orr_scope *s, int64_t cap, int64_t *out_ids /* host */, int64_t *out_n);
void    orr_scope_destroy(orr_scope *s);

/* orr_search_batch_masked with the scope taken from a handle: what orr_search_batch would return on a shard sealed from scratch
 * from only the scope's live rows, in their present candidate order -- rows, order and fp64 scores bit for bit.
 * candidate_limit counts the scope's live rows; an empty scope gives counts of 0; topk, dim 0 or another dimension, NaN order
 * and ties follow orr_search_batch.  Nothing is resolved: no id crosses to the device, no lookup and no count runs, and when
 * candidate_limit reaches every row of the scope not even the clip is computed.  The paths behind the resolve, "mask_screen",
 * "mask_part_rows" and the statistics (pass_mode 5 or 4) are the masked call's.
 * ORR_EINVAL: the masked call's argument errors, a NULL scope (before the index handle is looked at), a scope of another shard.
 * ORR_ESTATE: an orphaned scope. */
int orr_search_batch_in_scope(orr_index *idx, int32_t B, int32_t dim, const float *q,
                              const uint8_t *terms_utf8, const uint32_t *term_off, const uint32_t *query_term_off,
                              int64_t now_ticks, int32_t topk, int64_t candidate_limit, const orr_scope *scope,
                              int64_t *out_rows, double *out_scores, int32_t *out_counts);

/* orr_search_batch_masked_groups with the groups taken from handles: query b searches inside scopes[query_scope[b]], and its
 * result is what orr_search_batch_in_scope returns for it with that scope.  n_scopes is 1 .. 64; scopes may repeat, overlap, be
 * empty or be named by no query.  The scopes large enough to screen share one pass over the shard's shadow (pass_mode 6); the
 * others, and queries that pass cannot certify, run as the in-scope call of their handle.  One used scope IS the in-scope call.
 * ORR_EINVAL before any device call and before the index handle is looked at: n_scopes outside 1 .. 64, scopes or an entry of
 * it NULL, query_scope NULL or an entry outside [0, n_scopes); then: a scope of another shard.  ORR_ESTATE: an orphaned scope. */
int orr_search_batch_in_scopes(orr_index *idx, int32_t B, int32_t dim, const float *q,
                               const uint8_t *terms_utf8, const uint32_t *term_off, const uint32_t *query_term_off,
                               int64_t now_ticks, int32_t topk, int64_t candidate_limit,
                               int32_t n_scopes, const orr_scope *const *scopes, const int32_t *query_scope /* host [B] */,
                               int64_t *out_rows, double *out_scores, int32_t *out_counts);

/* ---- cosine range search -----------------------------------------------------
 * For each of B query vectors: EVERY row whose cosine to it is at least min_cosine[b], with that cosine -- the range question
 * beside top-k (near-duplicates at ingest, "more like this chunk, with scores", evidence checks above a similarity).  A search
 * ranks at most topk rows by the fused score; orr_scope_create_near makes a set without cosines for one threshold.
 *   a hit           row r is a hit of query b when it is live, it is in `within` (NULL: every live row) and
 *                   CosineSimilarity(q_b, e_r) >= min_cosine[b]: the reference's function (RecallSearchService.cs:69-88) bit for
 *                   bit, compared as C# compares doubles.  The guards are orr_scope_create_near's: a row without an embedding
 *                   has cosine 0, so has a query with norm <= 0, so has every pair when dim is 0 (q may be NULL) or differs
 *                   from the index's -- no row is walked for such a query: its hits are all the allowed rows in candidate order
 *                   when 0 >= min_cosine[b], and none otherwise.  A NaN cosine is never a hit.
 *   out_total [B]   the exact number of hits of each query
 *   out_n [B]       min(out_total[b], max_hits)
 *   out_hits        [B][max_hits]: out_hits[b][0 .. out_n[b]) are the best hits, cosine descending (as double.CompareTo orders)
 *                   and then candidate position ascending; cosine is the reference's double, order_key = row_base + position as
 *                   in orr_candidate.  The entries behind out_n[b] are not written.  max_hits == 0 asks for totals only
 *                   (out_hits may be NULL).
 *   B               1 .. 64; B == 0 returns ORR_OK and writes nothing.  q is [B][dim] floats in host or device memory.
 *   min_cosine      host [B], one threshold per query; -infinity and +infinity are allowed, NaN is ORR_EINVAL.
 * The call is for SELECTIVE thresholds.  Where dim % 128 == 0 and the int8 shadow fits (it is built at the first call, on a
 * shard of any size) the rows are screened through the shadow, four queries per stream, with a rigorous per-pair bound; the
 * surviving pairs are re-scored in the reference's arithmetic on the device and every pair that is not certainly below the
 * threshold is decided on the host by the host finish's own expression.  Other queries (another dim % 128, non-finite or tiny
 * coordinates: 0 < max|q| < 2^-48) take the exact form: the exact-dot walk of all rows, eight queries per walk.  Both give the
 * same answer.  When the pairs of ONE query that would have to be re-scored exceed "range_pair_cap" the call returns ORR_ELIMIT:
 * out_n is all 0, no hit is written, and out_total[b] holds for EVERY query the number of pairs that were kept for it -- an
 * upper bound of its hits, so the caller sees which query to tighten.  An unselective set is what orr_scope_create_near makes.
 * Options (orr_index_set_option): "range_pair_cap" 1 .. 2^31 (default 1,048,576); "range_buffer" 1 .. 4,194,240 (default
 * 8192), the entries per query the survivors' buffers and hit lists start with -- a call that needs more grows them to what it
 * measured and runs that launch group again, and the lane keeps the grown size: a list is never truncated; "range_form" 0 the
 * library's choice (today: the screen wherever it applies), 1 the screen wherever it applies, 2 the exact form only (for tests
 * and measurements: the answers are the same).
 * The call takes a search lane as orr_search_batch_in_scope does: re-entrant on one handle, views work, the scope is held shared
 * for the call.  The search statistics do not move; the kernel statistics record every launch under its own name
 * (screen_gemv_i8_range, range_rescore_exact, range_collect, range_dot_exact, range_collect_dense, ...) and, as byte counts
 * without launches, range_screen_pairs (16 bytes per pair the screen kept) and range_host_pairs (32 bytes per pair the host
 * decided).
 * Errors, in this order, before the handle is looked at and with the outputs untouched: ORR_EINVAL for B outside 0 .. 64, dim
 * negative, max_hits negative; then, for B > 0: q NULL with dim > 0, min_cosine NULL, out_hits NULL with max_hits > 0, out_n
 * NULL, out_total NULL, a NaN threshold; then a NULL index.  Then ORR_EINVAL for a scope of another shard, ORR_ESTATE for an
 * orphaned scope or an index that is not sealed. */
typedef struct orr_range_hit {
    int64_t row_id;         /* caller's id of the row                                           */
    int64_t order_key;      /* global candidate position (row_base + position in the shard)     */
    double  cosine;         /* CosineSimilarity(q_b, e_r), the reference's value                */
} orr_range_hit;            /* 24 bytes */
int orr_search_range_cosine(orr_index *idx, int32_t B, int32_t dim, const float *q /* host or device, [B][dim] */,
                            const double *min_cosine /* host [B] */, const orr_scope *within /* or NULL: every live row */,
                            int32_t max_hits, orr_range_hit *out_hits /* host [B][max_hits] */,
                            int32_t *out_n /* host [B] */, int64_t *out_total /* host [B] */);

/* orr_search_range_cosine for a BULK of queries: the same contract word for word, except that B is 0 .. 1024 -- the hits, their
 * order, the cosine bits, order_key and out_total, the guards, ORR_ELIMIT with its upper bounds, lanes, views and scopes, and the
 * argument errors in their order with the first rule reading 0 .. 1024.  For any batch the answer is exactly what
 * orr_search_range_cosine returns on the same queries in slices of 64 (an upload's hundreds of overlapping chunks against the
 * shard: the near-duplicate question at ingest in one call).
 * What differs is the screen.  Where dim % 128 == 0 and dim >= 512, the int8 shadow is in place and at least 65 queries of the
 * call are screened at all, they go through ONE pass of the int8 screening GEMM per launch group (kernel statistics:
 * screen_tile16_range, in front of it range_i8_tile_queries) with the bound for the query's first int8 level, instead of one
 * stream over the shard per four queries; a launch group is as many queries as their survivors' buffers fit in 2 GiB.  Every
 * other query goes where orr_search_range_cosine sends it: the stream in groups of four, or the exact form; with B <= 64 the
 * call launches what orr_search_range_cosine launches.  Option "range_gemm" (orr_index_set_option, sticky, this call only):
 * 0 the rule above (default), 1 the GEMM wherever its shape applies, from one query up, 2 never (for tests and measurements:
 * the answers are the same).  "range_form" 2 still sends everything to the exact form; "range_pair_cap" and "range_buffer" work
 * as they do there. */
int orr_search_range_cosine_bulk(orr_index *idx, int32_t B, int32_t dim, const float *q /* host or device, [B][dim] */,
                                 const double *min_cosine /* host [B] */, const orr_scope *within /* or NULL: every live row */,
                                 int32_t max_hits, orr_range_hit *out_hits /* host [B][max_hits] */,
                                 int32_t *out_n /* host [B] */, int64_t *out_total /* host [B] */);

/* ---- diverse search: the results compared WITH EACH OTHER ------------------------------------------------------------------
 * Every search above compares a query with rows.  This one also compares the best rows of a query with each other and returns
 * topk of them that are not near-copies of one another: a near-duplicate collapse of the ranked list, or maximal marginal
 * relevance (MMR).  The cluster form is orr_cluster_search_batch_diverse (with the other cluster calls, below); pools beyond 56
 * are not offered; a per-document cap is
 * orr_search_batch_per_key below.
 *
 * 1. The pool.  within == NULL: exactly what orr_search_batch returns for topk = pool; with a scope: exactly what
 *    orr_search_batch_in_scope returns for topk = pool -- rows, unrounded fused scores, order, and all their rules
 *    (candidate_limit, a foreign dim, ties, NaN order, deleted rows, lanes, views, a scope of another shard).
 *    max(1, topk) <= pool <= 56 (ORR_DIVERSE_MAX_POOL: the largest take the search serves from one selection list).
 *    DIVERSIFICATION NEVER LOOKS OUTSIDE THE POOL: when the pool runs out, out_counts[b] stays below topk.
 * 2. The cosines.  c_ij = CosineSimilarity(e_i, e_j) of RecallSearchService.cs:69-88 with the two STORED rows as a and b, bit for
 *    bit: evaluated on the host from three sums that are exact on the device.  A row without an embedding, or an index of
 *    dim 0, has cosine 0 with everything; the query's own dim plays no part.
 * 3. The greedy pass over the pool in rank order, on the host.
 *    ORR_DIVERSE_COLLAPSE, param = max_cosine: ranks 0, 1, ...; a member is kept unless c >= max_cosine (C#'s >=: a NaN cosine
 *      drops nothing) for some member already kept; stops at take = max(1, topk) kept.  max_cosine = +inf reads no cosine and
 *      gives the plain search's first `take` rows bit for bit.
 *    ORR_DIVERSE_MMR, param = lambda in [0, 1]: rank 0 is kept first; each next pick is the remaining member with the greatest
 *      (lambda * score) - ((1.0 - lambda) * m), binary64, left to right, no contraction; m is the maximum of its cosines to the
 *      kept members (the fold starts at -inf with `if (c > m) m = c`, so NaN is skipped; still -inf: m = 0).  Values are
 *      compared as double.CompareTo orders them, a tie goes to the lower pool rank.  With 1.0 - lambda == 0.0 the penalty is
 *      exactly 0: lambda = 1 is the plain search bit for bit and reads no cosine.
 * out_rows / out_scores [B][max(1,topk)]: the picks in pick order with their FUSED scores (not MMR values); out_counts [B];
 * out_pool_rank [B][max(1,topk)] (may be NULL): each pick's rank in the undiversified order.  Unused slots: -1 / 0.0 / -1.
 * ORR_EINVAL before the handle is looked at, the outputs untouched, in this order: out_rows, out_scores or out_counts NULL; pool
 * outside 1 .. 56; max(1, topk) > pool; a mode other than the two; param NaN; lambda outside [0, 1].  Then a NULL index, and,
 * unless B == 0 (which writes nothing), the errors of the underlying search.
 * Kernel statistics: the pool's search as always, then ONE pair_dots launch for (up to 1024 queries of) the batch; a query whose
 * pool has fewer than 2 members, an index of dim 0, max_cosine = +inf and lambda == 1 take none.  The search statistics move as
 * for one search of B queries. */
#define ORR_DIVERSE_COLLAPSE 0
#define ORR_DIVERSE_MMR      1
#define ORR_DIVERSE_MAX_POOL 56
int orr_search_batch_diverse(orr_index *idx, int32_t B, int32_t dim, const float *q,
                             const uint8_t *terms_utf8, const uint32_t *term_off, const uint32_t *query_term_off,
                             int64_t now_ticks, int32_t topk, int64_t candidate_limit,
                             const orr_scope *within /* or NULL: every live row */,
                             int32_t pool, int32_t mode, double param,
                             int64_t *out_rows, double *out_scores, int32_t *out_counts,
                             int32_t *out_pool_rank /* [B][max(1,topk)], may be NULL */);

/* ---- row keys and the per-key search: at most m rows per document, exact beyond the pool ------------------------------------
 * Every search above ranks chunks; a corpus cut by a sliding-window chunker lets one relevant document own the first ten places.
 * An orr_keys is a handle like orr_scope: one int64_t key per row of one sealed shard, resident on its device (8 bytes per row);
 * ORR_KEY_NONE means "no key".  A key is whatever the host groups by, typically a document number.
 *
 *   orr_keys_create  every row starts at ORR_KEY_NONE, then what orr_keys_set does.
 *   orr_keys_set     the ids are resolved through the id table exactly as orr_scope_create resolves them (host or device memory,
 *                    keys in the same memory as row_ids); keys[i] is stored at every live row of row_ids[i]; ids that name no
 *                    live row are passed over; *out_set (may be NULL) = the entries that named a live row.  For an id listed
 *                    twice with different keys the row gets one of them: it is UNSPECIFIED which.  n == 0 is legal.
 *   orr_keys_get     host ids -> host keys; an unknown or dead id reads ORR_KEY_NONE.
 *   orr_keys_rows    the live rows whose key is not ORR_KEY_NONE (one counting launch); -1 on an orphaned handle or NULL.
 *   orr_keys_destroy NULL is allowed.
 * Maintenance: orr_index_delete_rows and orr_index_update_rows need nothing; orr_index_compact and orr_index_insert_rows carry
 * every registered orr_keys through the move with ONE keys_remap launch per call, from the sources scope_remap reads; a new row
 * reads ORR_KEY_NONE until the host sets it.  Insertion allocates the grown columns in its allocation phase: ORR_ENOMEM leaves
 * shard, scopes and keys as they were.  Lifetime and threads are orr_scope's: registered with the owning index, usable through
 * any view, held shared by searches and exclusively by set and destroy; create, set, get and rows take a lane;
 * orr_index_destroy frees the device part and orphans the handle (ORR_ESTATE from then on, rows -1, destroy still frees the
 * host part).  Not saved in the shard file, like scopes.
 *
 * orr_scope_create_keys: "search inside these documents" without listing a chunk id -- the live rows whose key equals one of
 * keys[0 .. n_keys) (host; duplicates count once; listing ORR_KEY_NONE selects the rows without a key), an ordinary orr_scope
 * from then on.  n_keys 0 .. 65,536; 0 gives the empty scope.  One keys_member launch.  ORR_EINVAL in this order: out NULL,
 * n_keys outside its range, keys NULL with n_keys > 0, a NULL keys handle, a NULL index; then keys of another shard
 * (ORR_EINVAL) or orphaned (ORR_ESTATE).
 *
 * orr_search_batch_per_key.  Let R be the complete ranking of the call's candidates: what orr_search_batch (within == NULL) or
 * orr_search_batch_in_scope would return with topk = all rows -- rows, unrounded fused scores bit for bit, order, the NaN
 * order, candidate_limit counting live rows (of the scope).  Walk R from the top: a row is kept when its key is ORR_KEY_NONE or
 * fewer than max_per_key kept rows carry its key; stop at take = max(1, topk) kept.  out_rows / out_scores / out_keys
 * [B][take] in walk order, out_counts [B]; unused slots -1 / 0.0 / ORR_KEY_NONE.  THE CALL LOOKS OUTSIDE THE POOL:
 * out_counts[b] < take only when the candidates ran out.  max_per_key 1 .. INT32_MAX (at max_per_key >= take the result is the
 * plain search's first take rows bit for bit); max(1, topk) <= pool <= 56 as in the diverse search.
 * The rounds (csrc/orr_per_key_plan.h): round 1 is the plain (in-scope) search for topk = pool; a query whose walk has not
 * kept take rows goes on, in slices of at most 64 queries, to rounds over the FROZEN candidate set of round 1 without the rows
 * of closed keys (keys_exclude: 64 exclusion bitmaps in one pass over the rows) and without the rows already seen
 * (keys_clear_seen), with no further limit, the slice's scopes sharing ONE grouped search; one keys_gather per round reads the
 * rows' keys.  out_rounds [B] (may be NULL) = the rounds run, <= take.  The search statistics move as for the searches run.
 * ORR_EINVAL before the handle is looked at, the outputs untouched, in this order: out_rows, out_scores, out_keys or out_counts
 * NULL; pool outside 1 .. 56; max(1, topk) > pool; max_per_key < 1; keys NULL; then a NULL index, and, unless B == 0 (which
 * writes nothing), the errors of the underlying search.  Then ORR_EINVAL for a scope or keys of another shard, ORR_ESTATE for an
 * orphaned scope or keys.
 * Out of scope: the cluster forms (built since: orr_cluster_keys and orr_cluster_search_batch_per_key with the other cluster
 * calls, below) and sharded.py, the record (shard) form, the service mirror and the micro-batcher, saving
 * keys in the shard file, pools above 56, and combining with the diverse search. */
#define ORR_KEY_NONE INT64_MIN
typedef struct orr_keys orr_keys;
int     orr_keys_create(orr_index *idx, int64_t n, const int64_t *row_ids /* host or device */,
                        const int64_t *keys /* same memory as row_ids */, orr_keys **out);
int     orr_keys_set(orr_keys *k, int64_t n, const int64_t *row_ids, const int64_t *keys, int64_t *out_set /* may be NULL */);
int     orr_keys_get(orr_keys *k, int64_t n, const int64_t *row_ids /* host */, int64_t *out_keys /* host */);
int64_t orr_keys_rows(const orr_keys *k);
void    orr_keys_destroy(orr_keys *k);
int     orr_scope_create_keys(orr_index *idx, const orr_keys *k, int32_t n_keys, const int64_t *keys /* host */, orr_scope **out);
int orr_search_batch_per_key(orr_index *idx, int32_t B, int32_t dim, const float *q,
                             const uint8_t *terms_utf8, const uint32_t *term_off, const uint32_t *query_term_off,
                             int64_t now_ticks, int32_t topk, int64_t candidate_limit,
                             const orr_scope *within /* or NULL: every live row */,
                             const orr_keys *keys, int32_t max_per_key, int32_t pool,
                             int64_t *out_rows, double *out_scores, int64_t *out_keys, int32_t *out_counts,
                             int32_t *out_rounds /* [B], may be NULL */);

/* ---- key groups: row counts and centroid vectors per key, on the device -----------------------------------------------------
 * The calls above read a key from the document to its rows (a cap, a filter).  These read it the other way round: which keys a
 * set of rows carries and how many rows each (the facet list of a scope, with no id crossing the bus), and one vector per key,
 * the mean of its rows' fp32 embeddings ("documents like this one", routing, a document-level index, a probe for
 * orr_scope_create_near).  The rules are csrc/orr_key_groups_plan.h's.
 *
 * THE RULE, bit for bit.  The MEMBERS of key K are the live rows r with key[r] == K, inside `within` when a scope is given, in
 * candidate order (position ascending).  The PARTICIPATING members are those whose stored norm satisfies normB > 0.0: rows
 * without an embedding, zero vectors and rows whose norm is NaN take no part; rows with an infinite norm do.  Let
 * u_0 < u_1 < ... < u_{n-1} be the participating members, cut into BLOCKS OF 256 consecutive members (ORR_KEY_GROUPS_BLOCK ==
 * key_groups::kBlock: part of the contract, the bits depend on it):
 *     P_j[d] = (((+0.0 + (double)e[u_{256j}][d]) + (double)e[u_{256j+1}][d]) + ...)     fp64, in this order
 *     S[d]   = (((+0.0 + P_0[d]) + P_1[d]) + ...)                                       fp64, in block order
 *     c[d]   = (float)(S[d] / (double)n)    on the HOST, IEEE division, round to nearest even; n == 0: c[d] = +0.0f, S[d] = +0.0
 * The device forms S with plain fp64 adds (no FMA, no reassociation); infinities and NaN coordinates follow IEEE.
 *
 *   orr_keys_groups     the distinct keys other than ORR_KEY_NONE among the members, ascending as signed integers; out_rows = each
 *                       key's member count (ALL members, not only the participating ones); *out_total = the distinct keys,
 *                       *out_n = min(*out_total, cap) entries written.  cap == 0 asks for the total only (the arrays may be NULL).
 *   orr_keys_centroids  n_keys 0 .. 65,536 (0 writes nothing); listing ORR_KEY_NONE asks for the rows without a key; a key listed
 *                       twice is answered twice; a key with no participating member gives zeros and out_used 0.  out_used[i] = n.
 *                       dim must be the index's and greater than 0, else ORR_EDIM.  The fp64 sums are formed in slices of keys
 *                       (64 MiB of sums; sticky option "key_groups_slice": 0 this rule, 1 .. 65,536 keys per slice; the bits do
 *                       not depend on it).
 *   orr_scope_centroid  all rows of the scope as ONE group, under the same rule and with the same kernels.
 * Kernels: keys_pairs_count / keys_pairs (one pass each over the rows: the selected rows compacted, order kept, by ballot and
 * prefix), hipCUB's stable radix sort and run-length encode, keys_block_sums (one workgroup per block; reads each participating
 * row once) and keys_block_fold (keys of several blocks).  No atomics decide an order.
 * ORR_EINVAL before any handle is looked at, the outputs untouched, in this order -- groups: cap negative; out_n or out_total
 * NULL; out_keys or out_rows NULL with cap > 0; keys NULL.  centroids: n_keys outside its range; keys NULL with n_keys > 0;
 * out_used NULL with n_keys > 0; the keys handle NULL.  scope_centroid: out_used NULL; the scope NULL.  Then ORR_EINVAL for a
 * scope of another shard, ORR_ESTATE for an orphaned handle, ORR_EDIM.  Lifetime and threads are orr_keys_get's: the call takes
 * a lane, holds keys and scope shared and works through views.  The search statistics do not move; every launch appears in the
 * kernel statistics under its own name.
 * Out of scope: the cluster forms (built since: §8w, orr_cluster_keys_groups / orr_cluster_keys_centroids /
 * orr_cluster_scope_centroid below define the blocked order across shards; a host may still ask each shard through
 * orr_cluster_keys_shard, but such per-shard sums added up ARE NOT the single index's bits), a mean
 * of unit-normalised rows or a weighted mean, sharded.py, the service mirror and the micro-batcher, keys in the shard file, a
 * search call that ranks documents by centroid (built since: §8x, orr_keys_centroid_index below makes the centroids of all keys
 * the rows of an ordinary orr_index, which every search call then ranks). */
#define ORR_KEY_GROUPS_BLOCK 256
int orr_keys_groups(orr_keys *k, const orr_scope *within /* or NULL */, int64_t cap,
                    int64_t *out_keys /* host [cap] */, int64_t *out_rows /* host [cap] */,
                    int64_t *out_n, int64_t *out_total);
int orr_keys_centroids(orr_keys *k, const orr_scope *within /* or NULL */, int32_t n_keys, const int64_t *keys /* host */,
                       int32_t dim, float *out_centroids /* host [n_keys][dim], may be NULL */,
                       double *out_sums /* host [n_keys][dim], may be NULL */, int64_t *out_used /* host [n_keys] */);
int orr_scope_centroid(orr_scope *s, int32_t dim, float *out_centroid /* host [dim], may be NULL */,
                       double *out_sum /* host [dim], may be NULL */, int64_t *out_used);

/* ---- document index: one centroid row per key, built on the device; stored rows read back -----------------------------------
 * orr_keys_centroid_index builds a sealed orr_index whose rows are the centroids of ALL keys of a key column, entirely on the
 * device; search, range search, cosine scopes, diverse search, save / load and the maintenance calls then work on documents
 * unchanged: the result is an ordinary orr_index.  The rules are csrc/orr_centroid_index_plan.h's.
 *
 * THE CONTRACT IS A TWIN.  The returned index answers every call bit for bit like the index a host would build this way, on
 * the same device:
 *   1. orr_keys_groups(k, within, ...) for all distinct keys, ascending; ORR_KEY_NONE is never among them.
 *   2. orr_keys_centroids(k, within, those keys, ...), in as many calls as the 65,536 limit needs: the float centroids and out_used.
 *   3. Every key with out_used == 0 is dropped: *out_skipped counts the dropped keys, *out_docs the kept ones.
 *   4. For each kept key in ascending key order one row: embedding = that centroid, the bits of THE RULE above,
 *      (float)(S[d] / (double)n); created_ticks = the CreatedAt ticks of the key's first participating member in candidate order,
 *      the newest chunk that takes part; row_id = the key itself; content = empty, so a document's keyword score is 0.
 *   5. orr_index_create with the source's device and dim, orr_index_append of those rows, orr_index_seal.
 * Lifetime: the result is an independent, caller-owned index, freed with orr_index_destroy.  It is a snapshot: it is registered
 * with nothing, does not follow later maintenance of the source, and outlives the source.  The ordinary maintenance calls
 * refresh it.  On any error the partial index is destroyed and *out is not written.
 * ORR_EINVAL before any handle is looked at, in this order: out NULL; k NULL.  After that the errors of orr_keys_centroids, in
 * its order: ORR_EINVAL for a scope of another shard, ORR_ESTATE for an orphaned handle, ORR_EDIM for a source with dim == 0.
 * Locks and lanes are orr_keys_centroids'; the call works through views.
 * On the device: no sum and no centroid crosses the bus.  Only small per-key tables go to the host -- run keys, run lengths and
 * ticks, 8 bytes per key each.  The pairs (a mode of their own: the participating members, sorted by the key itself), the sort
 * and the run-length steps are orr_keys_centroids'; keys_block_sums and keys_block_fold run in slices of keys
 * (key_groups::slice_keys, "key_groups_slice"; the 65,536 limit does not apply); keys_centroid_finish divides a slice's fp64
 * sums by the member counts (plain IEEE fp64 division, round to nearest even: key_groups::finish_one, the host's expression),
 * writes the fp32 centroids of the kept keys densely and gathers their ticks (keys_first_ticks, folded into the launch); a
 * finished slice goes into the result through orr_index_append, device to device.
 * Out of scope: a cluster form (the host route over orr_cluster_keys_centroids remains), caller-supplied content per document
 * (titles for the keyword score), a routed two-level call (top-r documents, then search inside them: it composes from this
 * index, orr_scope_create_keys and orr_search_batch_in_scopes; built since: §8y, orr_search_batch_routed below), keeping
 * the derived index in step with the source automatically, sharded.py, the service mirror and the micro-batcher, keys in the shard file, a pinned return path for
 * orr_keys_centroids.
 *
 * orr_index_get_rows returns the stored fp32 embedding of each listed live row, bit for bit (a sealed index or a view).  An
 * unknown or deleted id gives zeros and found 0; a row without an embedding gives the stored zeros and found 1.  A wrong dim, or
 * a dim of 0, is ORR_EDIM.  The id lookup is orr_keys_get's, the gather is rows_gather in slices of at most 64 MiB of workspace;
 * the call takes a lane like orr_keys_get.  ORR_EINVAL before the handle is looked at: n negative; row_ids or out_emb NULL with
 * n > 0; idx NULL. */
int orr_keys_centroid_index(orr_keys *k, const orr_scope *within /* or NULL */, orr_index **out,
                            int64_t *out_docs /* may be NULL */, int64_t *out_skipped /* may be NULL */);
int orr_index_get_rows(orr_index *idx, int64_t n, const int64_t *row_ids /* host */, int32_t dim,
                       float *out_emb /* host [n][dim] */, uint8_t *out_found /* host [n], may be NULL */);

/* ---- routed search: the top documents by centroid, then the best chunks inside them --------------------------------------------
 * orr_search_batch_routed ranks the rows of `docs` (any sealed index whose row ids are keys of `keys`: normally the result of
 * orr_keys_centroid_index; it may live on another device, be a view, or be idx itself) for every query, keeps the best `route`
 * of them, and searches idx (the chunk index, `keys` a key column of it) only inside the rows that carry one of those keys.
 * The rules are csrc/orr_routed_plan.h's.
 *
 * THE CONTRACT IS A TWIN.  For each query b, rows, order, fp64 score bits and counts are exactly what a host gets this way:
 *   1. Route: orr_search_batch(docs, 1, dim, q_b, the query's own terms, now_ticks, topk = route, candidate_limit = every row of
 *      docs) gives D_b, the returned row ids in rank order, and n_b, their number.  out_route_keys[b][0 .. n_b) = D_b, the
 *      entries behind ORR_KEY_NONE; out_route_n[b] = n_b.  A document index without content gives keyword score 0; a host-built
 *      docs with titles as content routes by them too.
 *   2. Scope: S_b = orr_scope_create_keys(idx, keys, D_b without ORR_KEY_NONE), ANDed with `within` when one is given.  An id
 *      equal to ORR_KEY_NONE is reported in out_route_keys but selects no row.
 *   3. Search: orr_search_batch_in_scope(idx, 1, dim, q_b, terms_b, now_ticks, topk, candidate_limit, S_b): candidate_limit
 *      counts the live rows of S_b; an empty S_b gives count 0.
 * Outputs: out_rows / out_scores [B][max(1, topk)], out_counts [B], unused slots -1 / 0.0; out_route_keys [B][route] and
 * out_route_n [B] may be NULL.  route is 1 .. 1024.  B == 0 returns ORR_OK and writes nothing.
 * ORR_EINVAL before any handle is looked at, in this order: an output among out_rows, out_scores, out_counts NULL; route outside
 * its range; keys NULL; docs NULL.  Then the errors of the search's own arguments in their order, then ORR_EINVAL for a `keys` or
 * `within` of another shard than idx and ORR_ESTATE for an orphaned handle.  On any error no output is written.
 * Locks: the route step runs through orr_search_batch on docs and takes and releases its own lane before a lane of idx is taken:
 * the call never holds both, and docs == idx cannot deadlock.  The chunk step holds one lane of idx with `within` and `keys`
 * shared, as orr_search_batch_per_key does.
 * On the device: queries with the same set of routed keys share one slot; per slice of at most 64 distinct slots the sorted
 * union table of the slots' keys (16 bytes per entry) goes up, ONE keys_include launch writes the slots' bitmaps (a workgroup of
 * 2,048 rows none of which is routed stores zeros without reading the base), one scope_counts, one mask_clip_slots and one
 * synchronise make them temporary scopes that are never registered with the index, and ONE grouped pass (the masked pass for a
 * slice of one slot) searches them.  No keys_member pass, no registered scope and no per-query synchronise runs.  The search
 * statistics count the call as one grouped call.
 * Out of scope: a cluster form, the service mirror and the micro-batcher, a record (shard) form, caller-supplied document
 * content built on the device, keeping a document index in step with its source, combining with the diverse or the per-key
 * search, a public call that makes many key scopes at once. */
int orr_search_batch_routed(orr_index *docs, orr_index *idx, const orr_keys *keys, int32_t B, int32_t dim, const float *q,
                            const uint8_t *terms_utf8, const uint32_t *term_off, const uint32_t *query_term_off,
                            int64_t now_ticks, int32_t route, int32_t topk, int64_t candidate_limit,
                            const orr_scope *within /* a scope of idx, or NULL */,
                            int64_t *out_rows, double *out_scores, int32_t *out_counts,
                            int64_t *out_route_keys /* host [B][route], may be NULL */,
                            int32_t *out_route_n /* host [B], may be NULL */);

/* orr_search_shard_masked with the scope taken from a handle: the record form of orr_search_batch_in_scope, the shard half of
 * orr_cluster_search_batch_in_scope.  The contract is orr_search_shard_masked's, unchanged: [B][kprime+1] records and the
 * trailer, `pass` 0 / 1, topk, candidate_limit GLOBAL with scope_before the scope's live rows on the shards in front (read
 * there with orr_scope_rows: no count runs), the one in-call repeat of overflowed queries, pass_mode 5 or 4.  Nothing is
 * resolved: no id crosses to the device, no lookup and no count runs, and a limit that reaches every row of the scope on this
 * shard computes no clip either.
 * ORR_EINVAL before any device call, in this order: kprime < 1, topk < 0, pass outside {0, 1}, scope_before < 0, out NULL, a
 * NULL scope, then a NULL index and the batch's argument errors; then a scope of another shard.  ORR_ESTATE: an orphaned scope. */
int orr_search_shard_in_scope(orr_index *idx, int32_t B, int32_t dim, const float *q,
                              const uint8_t *terms_utf8, const uint32_t *term_off, const uint32_t *query_term_off,
                              int64_t now_ticks, int32_t kprime, int64_t candidate_limit, int32_t topk, int32_t pass,
                              const orr_scope *scope, int64_t scope_before, orr_candidate *out);

/* orr_search_batch_in_scopes in record form: the shard half of orr_cluster_search_batch_in_scopes, with the contract of
 * orr_search_shard_in_scope.  Query b's [kprime+1] records and trailer are those of a search inside scopes[query_scope[b]];
 * orr_merge_candidates(_ex) takes them unchanged.  candidate_limit is GLOBAL and scope_before[g] is scope g's live rows on the
 * shards in front (their handles' orr_scope_rows): min(live_g, max(0, max(1, candidate_limit) - scope_before[g])) rows of scope
 * g take part here.  ONE pass at the caller's kprime, no ladder inside but the one in-call repeat of queries whose survivors'
 * buffers overflowed (with buffers of the call's own: "survivor_capacity" does not change); `pass` 0 / 1 and topk as in the
 * masked shard form.  The scopes large enough to screen share one pass over the shard's shadow (pass_mode 6; the front of that
 * pass gathers the handles' bitmaps and clips them in one launch); a small scope, and every scope where the shared pass is not
 * eligible or does not pay, answers through orr_search_shard_in_scope's pass for its queries.  A query's trailer carries in
 * order_key the rows of its OWN scope that took part here, and behind the screen ORR_CAND_TWO_STAGE with the floor in norm_b;
 * a query whose scope lets no row take part here gets an empty record list.  With one used scope the records are
 * orr_search_shard_in_scope's, record for record.  n_scopes is 1 .. 64; scopes may repeat, overlap, be empty or be named by
 * no query.
 * ORR_EINVAL before any device call and before a handle is looked at, in this order: n_scopes outside 1 .. 64; scopes or an entry
 * of it NULL; query_scope NULL or an entry outside [0, n_scopes); scope_before NULL or a negative entry; kprime < 1, topk < 0,
 * pass outside {0, 1}, out NULL; then a NULL index and the batch's argument errors; then a scope of another shard.
 * ORR_ESTATE: an orphaned scope. */
int orr_search_shard_in_scopes(orr_index *idx, int32_t B, int32_t dim, const float *q,
                               const uint8_t *terms_utf8, const uint32_t *term_off, const uint32_t *query_term_off,
                               int64_t now_ticks, int32_t kprime, int64_t candidate_limit, int32_t topk, int32_t pass,
                               int32_t n_scopes, const orr_scope *const *scopes, const int32_t *query_scope /* host [B] */,
                               const int64_t *scope_before /* host [n_scopes] */, orr_candidate *out);

/* ---- tuning knobs ----------------------------------------------------------
 * Integer options of one index; unknown names are ORR_EINVAL.
 *   "dead_rows_before"  deleted rows in the shards in front of this one (default 0), see above.
 *   "max_lanes"      1..16 (default 4): searches that may run at once on this handle (see "threads" above); lanes that
 *                    exist are kept.
 *   "kw_hits_cap"    entries of the keyword chain's hit list, one per (distinct query term, vocabulary token containing it)
 *                    (default 16M = 384 MB at most).  A batch that needs more grows the list to the measured count and
 *                    repeats its pass; the option exists to pre-size it (or, in tests, to force that path).
 *   "mask_screen"    0/1/2 (default 0): how orr_search_batch_masked picks its pass -- 0 by the cost rule (the masked screen
 *                    when max(4 x queries, 128) x scoped rows >= rows in front of the scope's last row, else the list path), 1 the
 *                    masked screen whenever the pass is eligible, 2 never (the list path in parts).  The results are the
 *                    same; the option exists for measurements and tests.
 *   "mask_part_rows" 1..4,194,240 (default 4,194,240): the most scoped rows one part of orr_search_batch_masked's list
 *                    path takes.  Smaller values exist so that tests reach the multi-part path on a small shard.
 *   "range_pair_cap", "range_buffer", "range_form"   see orr_search_range_cosine; "range_gemm": orr_search_range_cosine_bulk.
 *   "shard_pass"     0/1/2 (default 0): which pass orr_search_shard runs -- 0 the library's choice, 1 the unfused
 *                    batched pass, 2 the reference-arithmetic pass over every row.  The caller of
 *                    orr_merge_candidates sets 2 for the repeat of a batch some query of which could not be certified.
 *   "shard_topk"     the caller's topK for orr_search_shard (default 0: unknown).  When set, the two-stage pass takes its
 *                    floor from the k-th best score of the sampled prefix instead of the k'-th: fewer survivors.
 *   "fuse_epilogue"  0/1 (default 0): batches > 64 queries over >= 196,608 rows score and filter
 *                    inside the GEMM epilogue instead of writing the dots to HBM.
 *   "two_stage"      0/1/2 (default 1): searches over >= 196,608 rows screen ALL rows with ONE low-precision
 *                    product, keep every (query,row) pair that could reach a lower bound of the query's k-th
 *                    best score, and re-score those in the reference arithmetic on the device.
 *                    1: the product reads a shadow copy of the embeddings, built at the first such search (or
 *                    now if the index is sealed and the option is set explicitly): int8 with one scale per row
 *                    and a per-pair error bound when dim % 128 == 0 (+25 % HBM; a stream for 1..4 queries, an
 *                    int8 MFMA GEMM for more), bf16 otherwise (+50 % HBM, bound 2^-7 |q||e|); silently falls
 *                    back to 2 when the shadow does not fit.  2: no shadow: 5+ queries convert the fp32 rows to
 *                    bf16 inside the kernel, fewer run the exact kernel.  0: exact kernel (1..4 queries) /
 *                    streaming or split-bf16 MFMA pass over all rows. */
int orr_index_set_option(orr_index *idx, const char *name, int64_t value);

/* Diagnostic: out[B][orr_index_rows] = the screening dots of the two-stage pass (fp32, host or device
 * memory), i.e. sum_k bf16(q_k) bf16(e_k) accumulated in fp32 on the matrix cores.  Lets a test check the
 * bound the pass relies on.  Needs the bf16 shadow (ORR_ENOMEM when it does not fit); dim % 64 == 0. */
int orr_index_screen_dots(orr_index *idx, int32_t B, int32_t dim, const float *q, float *out);

/* Diagnostic: the RAW int32 accumulators of the int8 screening GEMM (K2j), out_dots[B][orr_index_rows] (host or device), as
 * one FORM of the kernel computes them -- 0: eight-wave 32x32x32 tile (what batches of up to 64 queries, the sampled prefix
 * and the bf16 shadow run), 1: four-wave 32x32x32 tile (65..128 queries, very large shards), 2: four-wave 16x16x64 tile
 * (129+ queries: the dominant kernel of config C3/C5) -- with the same K loop, operand rings, request streams and persistent
 * walk of the output tiles as the fused launches of a search; only the scoring epilogue is replaced by a store.  nt_rows:
 * rows requested non-temporal (what a search does for batches of one query tile).  The integer work the screen does in
 * place of RecallSearchService.cs:77-82 is checkable bit for bit this way: out_iq[B][dim] / out_ie[rows][dim] (either may be
 * NULL) receive the quantised int8 images the product multiplies (queries: one level; rows: the shard's int8 shadow, untiled),
 * and out_dots must equal out_iq x out_ie^T exactly.  dim % 128 == 0; forms 1 and 2 need dim >= 448.  ORR_ENOMEM without room
 * for the shadow. */
int orr_index_screen_i8_dots(orr_index *idx, int32_t B, int32_t dim, const float *q, int32_t form, int32_t nt_rows,
                             int32_t *out_dots, int8_t *out_iq, int8_t *out_ie);

/* Diagnostics for the claims the screens' exactness rests on besides the GEMM's integers: every constant and every approximate
 * dot that a certificate charges can be compared with a high-precision restatement (tests/test_gpu_screen_bounds.py).
 * Out of scope of THESE entry points: the kernels that exist in fused form only (the bf16 stream K2g and the one-product bf16x1
 * form), and running a fused epilogue with a floor of zero.  Those, the floor a search screens against and what its fused
 * epilogue keeps are seen through orr_index_capture_screen below, inside a search itself (tests/test_gpu_screen_survivors.py).
 * Still out of scope: a pass in several row ranges (2M+ rows with query terms) is captured as the whole it is, the ranges'
 * launches are not told apart; the cluster forms capture per shard handle only.
 *
 * orr_index_screen_i8_consts: what the int8 shadow holds per row -- out_scale / out_rel_err / out_rel_hat [rows] and
 * out_rowf [rows][4] -- and, for the B given queries (B may be 0), what the searches' quantisation makes of them: out_s1 [B],
 * out_err2 [B] (both int8 levels), out_err2_level1 [B] (the first level only: the screening GEMM's) and out_iq2 [B][dim], the
 * second-level image (orr_index_screen_i8_dots returns the first).  Any output may be NULL.  dim % 128 == 0. */
int orr_index_screen_i8_consts(orr_index *idx, int32_t B, int32_t dim, const float *q, float *out_scale, float *out_rel_err,
                               float *out_rel_hat, float *out_rowf, float *out_s1, double *out_err2, double *out_err2_level1,
                               int8_t *out_iq2);

/* The RAW int32 accumulators of the streaming int8 screen (K2i), out_dots[B][2][orr_index_rows]: [b][0] = I1 (first query
 * level), [b][1] = I2 (second level), for B = 1..4 queries, from the same K loop, prefetch, cross-lane reduction and grid as a
 * search's launch; only the scoring tail is replaced by two stores.  unit16 = 0: the 128-row-unit form of the pass over all
 * rows; 1: the 16-row-unit form of the sampled prefix, which needs dim % 1024 == 0 (ORR_EINVAL otherwise). */
int orr_index_screen_i8_stream_dots(orr_index *idx, int32_t B, int32_t dim, const float *q, int32_t unit16, int32_t *out_dots);

/* out[B][orr_index_rows] = the fp32 dots of one of the batched pass's kernels over the fp32 rows.  kernel 0: the streaming f32
 * MFMA form (K2s), the queries sent in groups of 32 as the pass sends them (up to 16 queries and 17..32 run different kernels);
 * kernel 1: the queries split into bf16 hi/lo halves, then the unfused three-product split-bf16 GEMM.  dim % 64 == 0. */
int orr_index_pass_dots(orr_index *idx, int32_t kernel, int32_t B, int32_t dim, const float *q, float *out);

/* Diagnostic: the two-stage screen of a search, seen directly (tests/test_gpu_screen_survivors.py): the floor each query was
 * screened against and the survivors' buffers as the screen (and, in a masked or grouped search, the scope filter behind it) left
 * them, in front of the exact tail.
 *
 * orr_index_capture_screen(idx, 1) arms the handle: the FIRST pass through the two-stage screen of the next search on it --
 * plain, shard, masked, grouped or scoped, whatever the entry point -- synchronises its stream at that point and copies the
 * fields below to host memory the handle owns; the tail then runs as always.  One capture per arming: later passes of the same
 * call (the repeats of overflowed queries) and later searches record nothing until the handle is armed again, which also drops
 * the capture it holds.  enabled = 0 disarms and keeps what was captured.  The capture changes neither which kernels run nor
 * their arguments nor the records returned; unarmed, a pass pays one branch on the host.  Searching one handle from several
 * threads while it is armed is the caller's error: which of them is captured is not defined.  A view handle of the caller's
 * (orr_index_view) is armed and read on its own.  ORR_EINVAL: a NULL index; ORR_ESTATE: the index is not sealed.
 *
 * orr_index_captured_screen reports and fetches.  With all five arrays NULL it fills *info only: sizes first.  With all five
 * given, B and cap must equal info->B and info->cap of the capture held:
 *   out_floor_key [B]       the floor keys (key > floor_key <=> score >= F; 0: no floor, everything is kept)
 *   out_L [B]               L, the lower bound of the query's exact kth best score that the floor stands for (-inf: none)
 *   out_cnt [B]             pairs the screen counted per query; more than cap: the buffer overflowed and holds the first cap
 *   out_key / out_pos [B][cap]   the buffers' entries (slots at or beyond min(cnt, cap) are left as they are): the screen's key
 *                           of the pair -- all ones where it was kept without one -- and the row's position (candidate order)
 * ORR_EINVAL, in this order, before the handle is looked at and with nothing written: info NULL; some but not all of the arrays
 * NULL; arrays given with B <= 0 or cap == 0; a NULL index.  Then ORR_ESTATE: the index is not sealed, or nothing was captured
 * since the handle was armed; ORR_EINVAL: B or cap differ from the capture's (nothing written, info neither). */
typedef struct orr_screen_capture {
    int32_t B;              /* queries of the captured pass */
    int32_t kth;            /* the floor's rank: max(1, topK) */
    uint32_t cap;           /* entries per query of the survivors' buffers in that pass */
    int32_t screen;         /* the screen that ran: 1 screen_i8_fused, 2 screen_gemv_i8, 3 screen_gemv_bf16, 4 screen_bf16_fused,
                               5 gemm_dot_bf16x1_fused */
    int32_t tile_form;      /* screen 1: 0 eight-wave, 1 four-wave 32 x 32 x 32, 2 four-wave 16 x 16 x 64 tile; else -1 */
    int32_t scope;          /* 0 no scope mask, 1 one shared scope, 2 groups of scopes */
    int32_t floor_form;     /* the prefix's floor: 0 full ranking, 1 per-lane maxima, 2 wave maxima; -1: a stream's or a masked sample's own ranking */
    int32_t reserved;
    int64_t n;              /* participating rows: positions [0, n) were screened */
    int64_t prefix_rows;    /* rows [0, prefix_rows) gave the floor; with a scope: the first prefix_rows in-scope rows (grouped: at most) */
    double eps3;            /* bound of the keys the floor was selected from, as the floor's launch got it */
    double eps1;            /* bound of the screen's keys (0: the int8 forms add their per-pair bound inside the kernel) */
} orr_screen_capture;
int orr_index_capture_screen(orr_index *idx, int32_t enabled);
int orr_index_captured_screen(orr_index *idx, orr_screen_capture *info, int32_t B, uint32_t cap, uint64_t *out_floor_key, double *out_L,
                              uint32_t *out_cnt, uint64_t *out_key, uint32_t *out_pos);

/* Diagnostic: the pair matrices orr_search_batch_diverse forms its cosines from (tests/test_gpu_diverse.py).  List l is the
 * positions[list_off[l] .. list_off[l + 1]) (candidate order: order_key - row_base); out[l][i][j] = out[l][j][i] is the exact dot
 * of its rows i and j -- products rounded to binary32, summed in binary64 in index order, RecallSearchService.cs:77-82 -- and the
 * diagonal a row's exact self-dot.  A position may repeat.  Elements at or beyond a list's own length are left as they were.
 * ORR_EINVAL from the host, before any launch: out NULL, n_lists < 0, stride outside 1 .. 56, list_off or positions NULL, a
 * NULL index, list_off not starting at 0 or decreasing, a list longer than stride, a position outside [0, orr_index_rows).
 * An index of dim 0: zeros.  Kernel statistic: pair_dots, one launch per 1024 lists. */
int orr_index_pair_dots(orr_index *idx, int32_t n_lists, const uint32_t *list_off /* host [n_lists+1] */,
                        const int64_t *positions /* host */, int32_t stride /* >= the longest list, <= 56 */,
                        double *out /* host [n_lists][stride][stride] */);

/* Diagnostic: the keyword chain of a search, seen directly (tests/test_gpu_keyword_chain.py).  Runs the chain exactly as a
 * search for ONE query that owns all n_terms terms runs it -- vocabulary match, alias stage, posting expansion, the repeat with
 * a grown hit list when the list was too short, and the cleanup that leaves the lane as a search leaves it -- and returns what
 * the scoring kernels would read:
 *   out_bitmaps [n_terms][words]  uint32, host memory: bit r & 31 of word r >> 5 is set iff row r (candidate order) contains
 *                                 the term.  words = ((orr_index_rows + 31) / 32 + 3) / 4 * 4, the chain's own words_per_term;
 *                                 pass it as out_words_per_term (ORR_EINVAL when it differs).  A term whose bitmap is a stored
 *                                 token bitmap is returned from there: the caller cannot tell from the bits where they came
 *                                 from.  The bits are RAW: the positions of deleted rows are NOT cleared (posting lists keep
 *                                 them until compaction; a search drops such rows behind the scoring).
 *   out_alias [n_terms]           uint8, may be NULL: 1 where the term's only hit was a token with a stored bitmap.
 *   out_info [4]                  int64: [0] words, [1] the (term, token) hits of the final, untruncated run, [2] how many
 *                                 times the chain ran, [3] the short-token form that ran: 0 all-pairs, 1 lookup (both are
 *                                 the kernel statistic "vocab_match").
 * terms_utf8 / term_off as in orr_search_batch: term t is bytes [term_off[t], term_off[t + 1]).  1 .. 4096 terms, none empty,
 * all DISTINCT (ORR_EINVAL otherwise); a result of more than 2^30 bytes is refused (ORR_EINVAL).
 * form: -1 as a search would choose, 0 the all-pairs form, 1 the lookup form.  mid: -1 default, 0 sends the tokens of 17..32
 * bytes through the wave-per-token scan.  Both hold for this call only and go ahead of ORR_VOCAB_LOOKUP / ORR_VOCAB_MID.
 * The search statistics do not move; the kernel statistics record the launches.  ORR_ESTATE when the index is not sealed. */
int orr_index_keyword_bitmaps(orr_index *idx, int32_t n_terms, const uint8_t *terms_utf8, const uint32_t *term_off, int32_t form,
                              int32_t mid, int64_t out_words_per_term, uint32_t *out_bitmaps, uint8_t *out_alias, int64_t *out_info);

/* ---- measurement ---------------------------------------------------------*/
/* enabled: 0 off; 1 an event pair around every kernel; 2 only around the one launch per search that streams every row
 * (each pair costs a few microseconds of stream time, which a one-query search notices).  Also resets the counters. */
int orr_index_set_profiling(orr_index *idx, int32_t enabled);
int orr_index_kernel_stats(orr_index *idx, orr_kernel_stat *out, int32_t cap);  /* returns count */

int orr_index_search_stats(orr_index *idx, orr_search_stats *out, int32_t reset);  /* out may be NULL (reset only) */

/* ---- several GPUs behind one handle, in ONE process ------------------------------
 * The reference host is a single process with a singleton store (Program.cs:59,
 * IngestionServiceCollectionExtensions.cs:22-23); north_star keeps that host in C#.  An orr_cluster owns one
 * shard per entry of `devices` (the same ordinal may appear twice: two shards on one GPU) and answers
 * orr_cluster_search_batch exactly as one orr_index over all the rows would: every shard scores the whole batch on
 * its own device at once (one host thread per shard), the per-shard [B][k'+1] candidate records come back through
 * pinned host memory, the host merges and certifies them as orr_merge_candidates does and repeats only the queries
 * that could not be certified.  (Between PROCESSES the same records travel by one RCCL all-gather: sharded.py.)
 *   create            dim as in orr_config; capacity_rows_per_shard reserves device memory per shard (0: grow).
 *   shard(i)          borrowed handle for orr_index_append / orr_index_set_option / orr_index_delete_rows.  Shard i
 *                     must receive rows that are all at least as new as every row of shard i + 1 (partition the
 *                     store's rows by CreatedAtUtc, newest first; orr_cluster_seal checks it): the global candidate
 *                     order (InMemoryIngestionStore.cs:61) is then shard 0's rows, shard 1's, ...
 *   seal              seals every shard (concurrently) and places them in the global order (row_base).
 *   search_batch      arguments as orr_search_batch; q must be HOST memory (each device uploads it).  Row ids are
 *                     the ids given at append (default: position in the shard + its row_base at append time, i.e.
 *                     pass explicit row_ids when appending to a cluster).
 * Thread-safe: cluster searches from different threads run side by side (each shard half on a search lane of its shard,
 * host halves on persistent pool threads); seal and destroy are exclusive. */
typedef struct orr_cluster orr_cluster;
int        orr_cluster_create(const int32_t *devices, int32_t n_shards, int32_t dim, int64_t capacity_rows_per_shard,
                              orr_cluster **out);
void       orr_cluster_destroy(orr_cluster *c);
int32_t    orr_cluster_shards(const orr_cluster *c);
orr_index *orr_cluster_shard(orr_cluster *c, int32_t i);
int        orr_cluster_seal(orr_cluster *c);
int64_t    orr_cluster_rows(const orr_cluster *c);
int        orr_cluster_search_batch(orr_cluster *c, int32_t B, int32_t dim, const float *q_host,
                                    const uint8_t *terms_utf8, const uint32_t *term_off,
                                    const uint32_t *query_term_off, int64_t now_ticks, int32_t topk,
                                    int64_t candidate_limit, int64_t *out_rows, double *out_scores,
                                    int32_t *out_counts);
/* Search inside a scope over all shards: exactly what orr_search_batch_scoped / orr_search_batch_masked return on ONE index
 * that holds all the cluster's rows in the global candidate order -- rows, order and fp64 scores bit for bit; candidate_limit
 * counts scoped live rows over the whole cluster; an id carried by rows on different shards brings every live one of them.
 * q_host AND scope_ids (and scope_off) are HOST memory, every shard's device reads them: a device pointer is ORR_EINVAL.  A null
 * cluster or a bad scope argument (as documented for the single-index calls) is ORR_EINVAL with the outputs untouched, an
 * unsealed cluster ORR_ESTATE.
 * A call holds one search lane per shard from start to end.  Every shard counts the scope's live rows (orr_index_scope_count),
 * the host splits the limit (scope_before = the live rows on the shards in front), every shard answers at once with k' records
 * per query (orr_search_shard_scoped / orr_search_shard_masked, topk handed down), the host merges as orr_merge_candidates_ex
 * does, and only the queries it cannot certify repeat: k' x 4 while a selection list holds it, then (masked) the list path
 * (pass = 1), then k' x 4 up to the largest number of scoped rows any shard lets take part, where every scoped row is a record;
 * ORR_EDEVICE if a query is uncertified even there.  One merge gathers at most 1 GiB of records (wider rungs run in slices of
 * the queries).
 * orr_cluster_search_stats counts searches, queries, passes (one per repeat, whatever the number of shards) and requeried; the
 * shards' own orr_index_search_stats keep counting their passes.  The "exchange" option does NOT apply: the records of these
 * two calls always come back through pinned host memory. */
int        orr_cluster_search_batch_scoped(orr_cluster *c, int32_t B, int32_t dim, const float *q_host,
                                           const uint8_t *terms_utf8, const uint32_t *term_off,
                                           const uint32_t *query_term_off, int64_t now_ticks, int32_t topk,
                                           int64_t candidate_limit, int64_t n_scope_ids, const int64_t *scope_ids,
                                           const uint64_t *scope_off, int64_t *out_rows, double *out_scores,
                                           int32_t *out_counts);
int        orr_cluster_search_batch_masked(orr_cluster *c, int32_t B, int32_t dim, const float *q_host,
                                           const uint8_t *terms_utf8, const uint32_t *term_off,
                                           const uint32_t *query_term_off, int64_t now_ticks, int32_t topk,
                                           int64_t candidate_limit, int64_t n_scope_ids, const int64_t *scope_ids,
                                           int64_t *out_rows, double *out_scores, int32_t *out_counts);
int        orr_cluster_search_stats(orr_cluster *c, orr_search_stats *out, int32_t reset);
/* Integer options of a cluster; unknown names are ORR_EINVAL.
 *   "exchange"   0 (default): the per-shard [B][k'+1] candidate records come back through pinned host memory (every record is
 *                wanted in ONE address space, so nothing needs a collective); 1: every shard writes its records into a
 *                device buffer and ONE RCCL all-gather over xGMI (ncclAllGather, one communicator per shard device, grouped
 *                from one thread) brings all shards' records to every device; the merge reads device 0's gathered copy --
 *                the literal exchange of BASELINE.json's north_star in the form a single-process host can load.  librccl.so is
 *                bound at run time (dlopen): ORR_ECOMM when it cannot be loaded, ORR_EINVAL when two shards share a device
 *                (a communicator needs distinct devices).  A failure of a later collective switches the cluster back to 0
 *                and returns ORR_ECOMM for that search. */
int        orr_cluster_set_option(orr_cluster *c, const char *name, int64_t value);
/* orr_index_compact on every shard (concurrently), then the shards are placed in the global order again. */
int        orr_cluster_compact(orr_cluster *c, int64_t *out_removed);

/* orr_index_insert_rows into shard `shard`.  The rows must keep the order orr_cluster_seal checks (every row of shard i at
 * least as new as every row of shard i + 1): ORR_EINVAL otherwise, BEFORE anything is written.  Then the shards are placed in
 * the global order again (row_base, "dead_rows_before").  Exclusive against cluster searches. */
int        orr_cluster_insert_rows(orr_cluster *c, int32_t shard, int64_t n, int32_t dim, const float *emb,
                                   const int64_t *created_ticks, const uint8_t *content_lower,
                                   const uint64_t *content_off, const int64_t *row_ids, int64_t *out_inserted);

/* ---- cluster scope handles: keep a resolved scope on every shard -------------
 * An orr_cluster_scope is a set of rows of one sealed cluster, held as ONE orr_scope PER SHARD; each part is made on its shard
 * by the single-shard call of the same name, at once on all shards, and every per-shard rule above holds unchanged: how unknown
 * ids, ids listed twice and ids carried by several rows resolve; half-open tick windows with INT64_MIN / INT64_MAX as the open
 * ends; ORR_TERMS_ALL / ORR_TERMS_ANY, at most 256 terms, no empty term; deleted rows are never in a scope; rows inserted later
 * are in no scope.  An id carried by rows on two shards sets a bit on both.  If the creation fails on any shard the parts
 * already made are destroyed, *out is untouched and that error is returned.
 *   maintenance  nothing new: the parts are registered with their shards, so orr_index_delete_rows on orr_cluster_shard(i),
 *                orr_cluster_compact and orr_cluster_insert_rows carry them.  The cluster scope caches no count: rows and the
 *                search read every part's count when they are called.
 *   add_ids      orr_scope_add_ids on every shard; *out_added (may be NULL) is the sum over the shards
 *   combine      orr_scope_combine on every shard; scopes of two different clusters are ORR_EINVAL; src == dst is allowed
 *   rows         the sum over the shards; -1 on an orphaned handle (or NULL)
 *   row_ids      the ids of the live rows in the GLOBAL candidate order (shard 0's, then shard 1's, ...): every shard writes at
 *                the offset of the live counts of the shards in front of it.  *out_n = their number; nothing is written beyond
 *                cap; when cap is too small: ORR_EINVAL after *out_n is set, nothing written at all
 *   shard        part i, borrowed as orr_cluster_shard's result is (never destroy it; NULL out of range): for orr_scope_rows
 *                and orr_search_shard_in_scope
 *   destroy      frees it and its parts (NULL is allowed)
 * add_ids and combine hold every part exclusively for the whole call -- taken in ascending shard order, within a shard by the
 * single shard's rule (dst and src in address order) -- so a search sees the edit on all shards or on none.  If an edit fails
 * on some shard (a device error), some shards may hold it and others not: the call returns that error and the cluster scope is
 * orphaned, never left half-applied and searchable; make it again.
 * orr_cluster_destroy orphans the cluster scopes that are still alive: every later call on one is ORR_ESTATE, rows is -1, and
 * orr_cluster_scope_destroy still has to be called to free the host part.  The two destroys may be called from different
 * threads in either order (the library serialises them); every other call on a cluster scope must have returned before its
 * cluster is destroyed.  orr_index_destroy of a cluster's shard is not a supported call.
 * create, add_ids, combine, row_ids and the search run beside cluster searches (each takes one lane per shard, in shard order)
 * and are excluded by orr_cluster_compact, orr_cluster_insert_rows and orr_cluster_seal.
 * Argument errors come before any device call and before a handle is looked at, with the outputs untouched, in this order: out
 * pointer NULL (row_ids: cap negative, out_n NULL, out_ids NULL with cap > 0), negative counts, ids NULL with n_ids > 0, op
 * outside 0 .. 2; for create_terms: out NULL, n_terms outside 0 .. 256, terms_utf8 or term_off NULL with n_terms > 0, mode
 * outside 0 .. 1, an empty term or offsets that decrease; for create_near: orr_scope_create_near's, in its order; then a NULL
 * scope, then a NULL cluster; then ids or probes in device memory (ORR_EINVAL: every shard's device reads them), ORR_ESTATE for an unsealed cluster or an orphaned scope. */
typedef struct orr_cluster_scope orr_cluster_scope;   /* opaque: one orr_scope per shard of one sealed cluster */
int     orr_cluster_scope_create(orr_cluster *c, int64_t n_ids, const int64_t *ids /* HOST */, orr_cluster_scope **out);
int     orr_cluster_scope_create_ticks(orr_cluster *c, int64_t ticks_from, int64_t ticks_to, orr_cluster_scope **out);
int     orr_cluster_scope_create_terms(orr_cluster *c, int32_t n_terms, const uint8_t *terms_utf8 /* host */, const uint32_t *term_off /* host [n_terms+1] */,
                                       int32_t mode, orr_cluster_scope **out);
int     orr_cluster_scope_create_near(orr_cluster *c, int32_t n_probes, int32_t dim, const float *probes /* HOST */,
                                      double min_cosine, int32_t mode, orr_cluster_scope **out);
int     orr_cluster_scope_add_ids(orr_cluster_scope *s, int64_t n_ids, const int64_t *ids /* HOST */, int64_t *out_added);
int     orr_cluster_scope_combine(orr_cluster_scope *dst, int32_t op, const orr_cluster_scope *src);
int64_t orr_cluster_scope_rows(const orr_cluster_scope *s);
int     orr_cluster_scope_row_ids(orr_cluster_scope *s, int64_t cap, int64_t *out_ids /* HOST */, int64_t *out_n);
const orr_scope *orr_cluster_scope_shard(const orr_cluster_scope *s, int32_t i);
void    orr_cluster_scope_destroy(orr_cluster_scope *s);

/* orr_cluster_search_batch_masked with the scope taken from a handle: what orr_search_batch_in_scope returns on ONE index that
 * holds all the cluster's rows with the same set of rows as its scope -- rows, order and fp64 scores bit for bit.
 * candidate_limit counts the scope's live rows over the whole cluster; an empty scope gives counts of 0 with the outputs filled
 * as the masked call fills them.  No id list goes to any shard and NO count step runs: behind the lanes every part is taken
 * shared in ascending shard order, the live counts are read from the handles, the limit is split on those numbers, and every
 * shard answers through orr_search_shard_in_scope's pass.  The merge, the ladder, the slices and the statistics are the masked
 * cluster call's; the "exchange" option does not apply.
 * Errors, in this order, with the outputs untouched: ORR_EINVAL for B <= 0, dim < 0, q_host NULL with dim > 0, query_term_off
 * NULL, out_rows or out_scores NULL, a NULL scope, a NULL cluster, q_host in device memory; ORR_ESTATE for an unsealed cluster
 * or an orphaned scope; ORR_EINVAL for a scope of another cluster. */
int orr_cluster_search_batch_in_scope(orr_cluster *c, int32_t B, int32_t dim, const float *q_host,
                                      const uint8_t *terms_utf8, const uint32_t *term_off, const uint32_t *query_term_off,
                                      int64_t now_ticks, int32_t topk, int64_t candidate_limit,
                                      const orr_cluster_scope *scope,
                                      int64_t *out_rows, double *out_scores, int32_t *out_counts);

/* Several cluster scopes in one batch: query b searches inside scopes[query_scope[b]], and its rows, order and fp64 scores are
 * bit for bit what orr_cluster_search_batch_in_scope returns for it with that scope.  candidate_limit counts each scope's own
 * live rows over the whole cluster.  n_scopes is 1 .. 64; scopes may repeat (a handle listed twice is one group and is held
 * once), overlap, be empty or be named by no query; the results never depend on which path ran.
 * Behind the lanes the parts of all distinct scopes are taken shared in one total order (ascending shard, within a shard
 * ascending part address), the live counts are read from the handles (no count step), the limit is split per scope, and every
 * shard runs orr_search_shard_in_scopes ONCE for the whole batch: the shards stream their shadows once per batch, not once per
 * scope.  A query the merge cannot certify repeats through the in-scope cluster ladder of its own scope, together with that
 * scope's other uncertified queries.  One used scope IS orr_cluster_search_batch_in_scope.  orr_cluster_search_stats reports
 * pass_mode 6 when a shard ran the shared pass; passes and requeried count as in the in-scope call.
 * Errors, in this order, with the outputs untouched: ORR_EINVAL for n_scopes outside 1 .. 64; scopes or an entry of it NULL;
 * query_scope NULL or an entry outside [0, n_scopes); B <= 0, dim < 0, q_host NULL with dim > 0, query_term_off NULL, out_rows
 * or out_scores NULL; a NULL cluster; q_host in device memory.  ORR_ESTATE for an unsealed cluster or an orphaned scope;
 * ORR_EINVAL for a scope of another cluster. */
int orr_cluster_search_batch_in_scopes(orr_cluster *c, int32_t B, int32_t dim, const float *q_host,
                                       const uint8_t *terms_utf8, const uint32_t *term_off, const uint32_t *query_term_off,
                                       int64_t now_ticks, int32_t topk, int64_t candidate_limit,
                                       int32_t n_scopes, const orr_cluster_scope *const *scopes, const int32_t *query_scope /* host [B] */,
                                       int64_t *out_rows, double *out_scores, int32_t *out_counts);

/* orr_search_range_cosine over a cluster: the answers of that call on ONE index holding all the cluster's rows -- ids, order,
 * cosine bits and totals.  Every shard runs the call at once on a lane of its own (taken in ascending shard order, the parts of
 * `within` held shared); the host merges the shards' lists by (cosine descending, order_key ascending), sums the totals and
 * cuts at max_hits.  ORR_ELIMIT from any shard is the call's status, with the shards' counts summed in out_total.  The options
 * are the shards' (orr_cluster_shard + orr_index_set_option).
 * Errors: orr_search_range_cosine's argument errors in its order, then a NULL cluster, then q_host in device memory
 * (ORR_EINVAL: every shard's device reads it); ORR_ESTATE for an unsealed cluster or an orphaned scope; ORR_EINVAL for a scope
 * of another cluster. */
int orr_cluster_search_range_cosine(orr_cluster *c, int32_t B, int32_t dim, const float *q_host, const double *min_cosine /* host [B] */,
                                    const orr_cluster_scope *within /* or NULL */, int32_t max_hits, orr_range_hit *out_hits,
                                    int32_t *out_n, int64_t *out_total);

/* orr_search_range_cosine_bulk over a cluster: orr_cluster_search_range_cosine with B 0 .. 1024, every shard running the bulk
 * call at once on its own lane; the lists are merged and the totals summed as there, and any shard's ORR_ELIMIT is the call's.
 * "range_gemm" is each shard index's own option. */
int orr_cluster_search_range_cosine_bulk(orr_cluster *c, int32_t B, int32_t dim, const float *q_host, const double *min_cosine /* host [B] */,
                                    const orr_cluster_scope *within /* or NULL */, int32_t max_hits, orr_range_hit *out_hits,
                                    int32_t *out_n, int64_t *out_total);

/* ---- diverse search over the shards ------------------------------------------------------------------------------------------
 * orr_search_batch_diverse on a cluster: exactly what that call returns on ONE index holding all the cluster's rows in the global
 * candidate order (with `within`: an index holding the same rows, scoped to the same set) -- rows, unrounded fused score bits,
 * counts, pool ranks, unused slots and every rule of the greedy pass.
 *   The pool is orr_cluster_search_batch (with a scope: orr_cluster_search_batch_in_scope) for topk = pool, with all their rules:
 *   the global candidate_limit, the ladder, an id carried by rows of several shards.  q_host is host memory.
 *   The cosines need two stored rows on one device, and a pool usually spans shards.  Each query's HOME shard is the one that
 *   holds most of its pool (a tie: the lowest shard); the other members' rows are gathered on their shards (kernel statistic
 *   rows_gather, at most one launch per source shard and group), travel through pinned host memory into the home's staging
 *   buffer, and ONE pair_dots launch per home shard and group reads each row where it lies.  A pool of n members over G shards
 *   moves at most n - ceil(n / G) rows, a pool on one shard none.  A group is the consecutive queries whose staged rows fit
 *   64 MiB (at most 1024 per home).  Every sum is the single index's: a pair's dot does not depend on where its rows lie.
 *   max_cosine = +inf, lambda == 1, a pool of fewer than 2 rows and a cluster of dim 0 read no cosine, launch nothing beyond the
 *   pool's search and give the cluster search's first max(1, topk) rows bit for bit.
 * ORR_EINVAL before any handle is looked at, the outputs untouched, in orr_search_batch_diverse's order; then a NULL cluster;
 * then, unless B == 0 (which writes nothing): an unsealed cluster (ORR_ESTATE), a scope of another cluster (ORR_EINVAL) or an
 * orphaned one (ORR_ESTATE), the errors of the underlying cluster search.  The cluster's search statistics move as for one
 * search of B queries.  The call holds the cluster shared from the pool's search to the last matrix (orr_cluster_compact and
 * orr_cluster_insert_rows wait for it).  Not offered: the record (shard) form, pools above 56, a peer-to-peer or RCCL transport
 * of the rows (the cluster per-key search: built since, orr_cluster_search_batch_per_key below). */
int orr_cluster_search_batch_diverse(orr_cluster *c, int32_t B, int32_t dim, const float *q_host,
                                     const uint8_t *terms_utf8, const uint32_t *term_off, const uint32_t *query_term_off,
                                     int64_t now_ticks, int32_t topk, int64_t candidate_limit,
                                     const orr_cluster_scope *within /* or NULL: every live row */,
                                     int32_t pool, int32_t mode, double param,
                                     int64_t *out_rows, double *out_scores, int32_t *out_counts,
                                     int32_t *out_pool_rank /* [B][max(1,topk)], may be NULL */);

/* Diagnostic: orr_index_pair_dots over a cluster (tests/test_gpu_cluster_diverse.py).  The lists are of GLOBAL order keys
 * (row_base of the shard + position); every list goes through the plan and the two kernels of orr_cluster_search_batch_diverse,
 * and out is what orr_index_pair_dots writes on one index holding all the rows, bit for bit.  ORR_EINVAL from the host, before
 * any launch, in that call's order; then a NULL cluster, a malformed list_off, an unsealed cluster (ORR_ESTATE), an order key
 * outside every shard.  A cluster of dim 0: zeros. */
int orr_cluster_pair_dots(orr_cluster *c, int32_t n_lists, const uint32_t *list_off /* host [n_lists+1] */,
                          const int64_t *order_keys /* host */, int32_t stride /* >= the longest list, <= 56 */,
                          double *out /* host [n_lists][stride][stride] */);

/* ---- row keys and the per-key search over the shards ----------------------------------------------------------------------------
 * An orr_cluster_keys is to orr_keys what orr_cluster_scope is to orr_scope: one orr_keys per shard of one sealed cluster, each
 * made on its shard and registered there, so orr_index_delete_rows / orr_index_update_rows on a shard, orr_cluster_compact and
 * orr_cluster_insert_rows carry it with no code of their own (a new row reads ORR_KEY_NONE until the host sets it).  The cluster
 * owns the handle: orr_cluster_destroy orphans it (ORR_ESTATE from then on, rows -1), and both destroy orders are legal.
 *
 *   orr_cluster_keys_create  row_ids and keys are HOST memory (every shard's device reads them); every row starts at ORR_KEY_NONE,
 *                            then what orr_cluster_keys_set does.
 *   orr_cluster_keys_set     the whole list goes to every shard at once; a shard passes over the ids it does not hold.  *out_set
 *                            (may be NULL) is the SUM of the shards' counts: AN ID THAT IS LIVE ON TWO SHARDS COUNTS TWICE (every
 *                            row of it gets the key).  All parts are taken under one hold, so a search sees an edit on every shard
 *                            or on none; an edit that fails on some shards orphans the handle.
 *   orr_cluster_keys_get     host ids -> host keys: per id the answer of the LOWEST shard whose answer is not ORR_KEY_NONE, else
 *                            ORR_KEY_NONE.
 *   orr_cluster_keys_rows    the sum of the parts' orr_keys_rows; -1 on NULL or an orphaned handle.
 *   orr_cluster_keys_shard   shard i's part, borrowed (like orr_cluster_shard): never destroy it; NULL for a bad index.
 *   orr_cluster_keys_destroy NULL is allowed.
 *   orr_cluster_scope_create_keys  orr_scope_create_keys on every part; the result is an ordinary orr_cluster_scope.  ORR_EINVAL
 *                            in that call's order (out NULL, n_keys outside 0 .. 65,536, keys NULL with n_keys > 0, a NULL keys
 *                            handle), then a NULL cluster, keys of another cluster (ORR_EINVAL) or orphaned (ORR_ESTATE).
 *
 * orr_cluster_search_batch_per_key returns what orr_search_batch_per_key returns on ONE index holding all the cluster's rows in
 * the global candidate order: rows, unrounded fused score bits, keys, counts, out_rounds, unused slots -1 / 0.0 / ORR_KEY_NONE,
 * and every rule of that call -- it looks outside the pool, so out_counts[b] < take only when the candidates ran out.
 *   Round 1 is orr_cluster_search_batch (with `within`: orr_cluster_search_batch_in_scope) for topk = pool.  Every pool member is
 *   a global order key; each shard that holds members reads their keys with ONE keys_gather, and a batch that finishes here
 *   launches nothing else.  The frozen candidate set of round 1 is built per shard, once, when a second round is first needed:
 *   without a scope the shard's part of the global candidate_limit prefix, with one the shard's share of max(1, candidate_limit)
 *   scoped live rows (the split of the in-scope cluster search), a partly covered shard clipped at its share.  A later round, per
 *   slice of at most 64 unfinished queries: the union table of the slice's closed keys goes to EVERY shard (a key closes
 *   cluster-wide: its rows may lie anywhere), each seen position to the shard that holds it; every shard at once runs one
 *   keys_exclude, at most one keys_clear_seen, one scope_counts and one mask_clip_slots; ONE grouped cluster search (the in-scope
 *   search for a slice of one query) runs over the slice's temporary scopes at topk = pool with no further limit.  The rules that
 *   are new are csrc/orr_cluster_per_key_plan.h's.
 *   The call holds the cluster shared from round 1 to the last round (orr_cluster_compact and orr_cluster_insert_rows wait for
 *   it), ONE set of lanes, taken in ascending shard order, for everything behind round 1 (with `within`: from round 1 on), and
 *   behind the lanes the keys' and the scope's parts shared in one total order.  The cluster's search statistics move by one
 *   search of B queries for round 1 and by one search of S queries per slice and round after that.
 * ORR_EINVAL before any handle is looked at, the outputs untouched, in orr_search_batch_per_key's order (an output NULL; pool
 * outside 1 .. 56; max(1, topk) > pool; max_per_key < 1; keys NULL); then a NULL cluster; then, unless B == 0 (which writes
 * nothing): an unsealed cluster (ORR_ESTATE), keys or a scope of another cluster (ORR_EINVAL), orphaned keys or scope
 * (ORR_ESTATE), q_host in device memory (ORR_EINVAL: every shard's device reads it), the errors of the underlying search.
 * Out of scope: sharded.py, the record (shard) form, the service mirror and the micro-batcher, keys in the shard file, pools above
 * 56, combining with the diverse search, de-duplicating the union table per shard. */
typedef struct orr_cluster_keys orr_cluster_keys;
int       orr_cluster_keys_create(orr_cluster *c, int64_t n, const int64_t *row_ids /* HOST */, const int64_t *keys /* HOST */, orr_cluster_keys **out);
int       orr_cluster_keys_set(orr_cluster_keys *k, int64_t n, const int64_t *row_ids, const int64_t *keys, int64_t *out_set /* may be NULL */);
int       orr_cluster_keys_get(orr_cluster_keys *k, int64_t n, const int64_t *row_ids, int64_t *out_keys);
int64_t   orr_cluster_keys_rows(const orr_cluster_keys *k);
orr_keys *orr_cluster_keys_shard(orr_cluster_keys *k, int32_t shard);          /* borrowed, like orr_cluster_scope_shard */
void      orr_cluster_keys_destroy(orr_cluster_keys *k);
int       orr_cluster_scope_create_keys(orr_cluster *c, const orr_cluster_keys *k, int32_t n_keys, const int64_t *keys /* HOST */, orr_cluster_scope **out);
int       orr_cluster_search_batch_per_key(orr_cluster *c, int32_t B, int32_t dim, const float *q_host,
              const uint8_t *terms_utf8, const uint32_t *term_off, const uint32_t *query_term_off,
              int64_t now_ticks, int32_t topk, int64_t candidate_limit,
              const orr_cluster_scope *within /* or NULL */, const orr_cluster_keys *keys, int32_t max_per_key, int32_t pool,
              int64_t *out_rows, double *out_scores, int64_t *out_keys, int32_t *out_counts, int32_t *out_rounds /* may be NULL */);

/* ---- cluster key groups: row counts and centroid vectors per key across the shards ----------------------------------------------
 * The three key-groups calls for an orr_cluster.  The contract is the earlier cluster forms': THE ANSWERS OF THE SINGLE-INDEX CALL
 * ON ONE INDEX HOLDING ALL THE CLUSTER'S ROWS IN THE GLOBAL CANDIDATE ORDER (shard 0's rows, then shard 1's, ...), BIT FOR BIT --
 * keys, counts, fp64 sums, fp32 centroids, out_used.  A document cut by a shard border is the normal case (the cuts fall by row
 * count), and per-shard sums added up are not these bits, so the library carries the blocked order across the borders itself.
 * The rules that are new are csrc/orr_cluster_key_groups_plan.h's.
 *
 * THE RULE ACROSS SHARDS, bit for bit.  The single-index rule stays: the participating members (normB > 0.0) of key K, in order,
 * are cut into blocks of 256; P_j is the fp64 sum of block j in member order from +0.0; S is the fp64 sum of the P_j in block order
 * from +0.0; c = (float)(S / n) on the host.  On a cluster K's members are shard 0's in position order, then shard 1's, ...; for
 * shard g, count_g is K's participating members there, before_g their number on the shards in front, total their sum.  BLOCKS ARE
 * COUNTED FROM THE KEY'S FIRST MEMBER ANYWHERE, so a block may straddle a border:
 *   head      before_g % 256 != 0: the first min(count_g, 256 - before_g % 256) members continue the block left open in front of
 *             this shard; their running sum starts from that block's carry P, not from +0.0.
 *   free      the members behind the head are cut into blocks of 256 from +0.0 (exactly keys_block_sums' blocks).
 *   closing   a block closes on the shard where its 256th member lies, or the key's last member.  Closed blocks are added to the
 *             running S in block order; S starts at +0.0 on the key's first shard and otherwise continues from the S the shard in
 *             front left.  A block still open at the end of a shard is not folded: its partial sum is the carry P for the next
 *             shard that holds a member.  A shard without a member of K is skipped; the carry passes over it.
 * Both carries are real data dependencies (fp64 addition is not associative); they concern one block and one running row per
 * spanning key and border.  Everything else -- all free blocks, every key that lies on one shard -- runs on every shard at once
 * through the single index's kernels and records.
 *
 *   orr_cluster_keys_groups     orr_keys_groups per shard, the shards' ascending lists merged on the host (rows of equal keys added).
 *   orr_cluster_keys_centroids  keys is HOST memory.  Every shard at once: keys_pairs_count / keys_pairs / the sort / keys_runs, one
 *                               sorted table for the call.  Per slice of keys ("key_groups_slice" of shard 0; the bits do not
 *                               depend on it), every shard at once: keys_block_sums, and keys_block_fold for keys wholly there; then
 *                               the shards in ascending order, only where a spanning key of the slice has members: ONE
 *                               keys_chain_step, its state (S and P, 2 x dim fp64 per spanning key) through one pinned host buffer.
 *                               A cluster cut between documents launches no keys_chain_step.  The finish is the host's, n = total.
 *   orr_cluster_scope_centroid  all rows of the cluster scope as ONE group, the same way.
 * Outputs, limits and special cases are the single-index calls': 0 .. 65,536 keys, ORR_KEY_NONE asks for the rows without a key, a
 * key listed twice is answered twice, no participating member gives zeros and out_used 0, cap == 0 asks for the total, out_used
 * is the key's participating count over the whole cluster.
 * Errors, in this order: ORR_EINVAL in the single-index calls' order before any handle is looked at, the outputs untouched; an
 * orphaned handle: ORR_ESTATE; keys and scope of different clusters: ORR_EINVAL; a foreign or non-positive dim: ORR_EDIM.
 * The call holds the cluster shared, one lane per shard taken in ascending shard order before any shard starts, and on each shard
 * the scope part's lock, then the keys part's shared lock.  The search statistics do not move; every launch appears in its shard's
 * kernel statistics under its own name.
 * Out of scope: sharded.py, the record (shard) form, the service mirror and the micro-batcher, keys in the shard file, a device-side
 * finish or a pinned return path for the sums, overlapping the chain of one slice with the free blocks of the next, a search that
 * ranks documents by centroid.  A key assignment that puts every key on every shard is answered correctly, at 2 x dim x 8 bytes of
 * state per key and border each way. */
int orr_cluster_keys_groups(orr_cluster_keys *k, const orr_cluster_scope *within /* or NULL */, int64_t cap,
                            int64_t *out_keys /* host [cap] */, int64_t *out_rows /* host [cap] */,
                            int64_t *out_n, int64_t *out_total);
int orr_cluster_keys_centroids(orr_cluster_keys *k, const orr_cluster_scope *within /* or NULL */, int32_t n_keys,
                               const int64_t *keys /* HOST */, int32_t dim, float *out_centroids /* host [n_keys][dim], may be NULL */,
                               double *out_sums /* host [n_keys][dim], may be NULL */, int64_t *out_used /* host [n_keys] */);
int orr_cluster_scope_centroid(orr_cluster_scope *s, int32_t dim, float *out_centroid /* host [dim], may be NULL */,
                               double *out_sum /* host [dim], may be NULL */, int64_t *out_used);

#ifdef __cplusplus
}
#endif
#endif /* OMNIRECALL_HIP_H */
