// host_ctx.inc -- part of uvaia_gpu.hip (included there, not a translation unit of its own): what the host side owns -- the tile stores and
// counter buffers made of the move-only handles of host_owners.h (device buffers, pinned blocks, events, streams) -- and the context.  Everything a
// context holds is released by its destructor: uvaia_gpu_close waits for the streams, unmaps what it mapped from other processes and deletes.

struct uvaia_gpu_ctx;

namespace {

thread_local std::string g_open_error;

int fail(uvaia_gpu_ctx *c, int code, const char *fmt, ...);

// One check for every HIP call; what happens on failure is the caller's hook (the code maps out-of-memory to UVAIA_GPU_ENOMEM).
#define HIP_TRY(call, on_fail) do { hipError_t e_ = (call); if (e_ != hipSuccess) { const int code_ = e_ == hipErrorOutOfMemory ? UVAIA_GPU_ENOMEM : UVAIA_GPU_EHIP; (void)code_; on_fail; } } while (0)
// what HIPCHK (host_owners.h) does on failure, in an entry point that has a context (or none: the message goes where
// uvaia_gpu_last_error(NULL) finds it) and in the handles: message, return the code
inline int hip_failed(uvaia_gpu_ctx *c, hipError_t e, const char *call, const char *file, int line)
{ return fail(c, e == hipErrorOutOfMemory ? UVAIA_GPU_ENOMEM : UVAIA_GPU_EHIP, "%s failed: %s (%s:%d)", call, hipGetErrorString(e), file, line); }

// the same for the FASTA parser's handle (host_fasta.inc), which is no context
int fasta_fail(uvaia_gpu_fasta *f, int code, const char *fmt, ...);
inline int hip_failed(uvaia_gpu_fasta *f, hipError_t e, const char *call, const char *file, int line)
{ return fasta_fail(f, e == hipErrorOutOfMemory ? UVAIA_GPU_ENOMEM : UVAIA_GPU_EHIP, "%s failed: %s (%s:%d)", call, hipGetErrorString(e), file, line); }
// (a plain nullptr stays what it was: no context yet, the message of a failed uvaia_gpu_open)
inline int hip_failed(std::nullptr_t, hipError_t e, const char *call, const char *file, int line)
{ return hip_failed(static_cast<uvaia_gpu_ctx *>(nullptr), e, call, file, line); }

}  // namespace

#include "host_owners.h"

namespace {

struct ScanEvt { Event a, b; double bytes = 0; };

// A set of reference tiles and what belongs to them: the buffers of a streamed batch and the resident database
struct TileStore {
  DevBuf<uint4> planes;          // packed tiles (allocated last: its presence says all of them are there)
  DevBuf<int> nonn;              // per reference: non-N sites
  DevBuf<int> amb;               // [AMB_ROW] per reference: side rows, the ambiguity-word lists of the references (as tab.d_amb_q for the queries)
  DevBuf<int> tot;               // per reference: valid sites (default) / ACGT sites (--acgt), counted by pack_refs_kernel
  // planes derived for the query set (column-compressed scan)
  DevBuf<uint4> ev, poly;
  DevBuf<uint32_t> grp;          // [tile][W4][64]  popc(E) | popc(V) << 16 of each word group (for queries that are all-N there)
  DevBuf<int> tote;
};

// One counter buffer of the resident search: what the scan of a slice leaves for its replay, and the events between the two
struct SliceBuf {
  DevBuf<uint32_t> cnt;          // [rows][ppad] two-counter scan output, one dword per pair: first | second << 16 (buffer 0: allocated at open for a pool, [nq_pad][pool_pad]; the others on first use);
                                 // its capacity is the pairs the buffer holds (grown when a slice needs more: slices may exceed a pool, see plan_subslices)
  DevBuf<int2> tmin;             // per (query, tile of 64 references): {smallest mismatch count, largest ACGT-match count}
  DevBuf<uint32_t> ext;          // packed-plane scan, default mode: per pair the other two counters (scan2_extras); sized like cnt
  DevBuf<uint32_t> rtp;          // ... and per reference the consensus pre-score packed into one dword (query sets with constant-and-complete columns)
  DevBuf<uint4> tb8;             // ... and per (query, tile of 64) the eight-entry bounds replay3_kernel walks (tile_bounds8)
  DevBuf<int4> rt;               // per reference of a slice: untruncated consensus pre-score (query sets with constant-and-complete columns)
  int tiles = 0, rb = 0, re = 0; long long tf = 0;     // the slice scanned into it: tiles, first and end reference relative to its first tile, that tile
  bool scanned = false, cons_done = false;
  Event scan_done, replay_done;
  bool replay_recorded = false;
};

}  // namespace

// Members are destroyed last to first: the streams come first so that they outlive every buffer and event that work queued on them may
// still name (uvaia_gpu_close has waited for them by then).
struct uvaia_gpu_ctx {
  int device = 0;
  // ---- streams, and what orders work between them
  struct Streams {
    Stream stream;
    Stream scan_streams[3];                 // the scan streams: small launches (few active query tiles) overlap on up to three streams; ring mode: scans of
                                            // later slices run on the first while the replay chain waits
    unsigned scan_rr = 0;
    int scan_nstreams = 1;                  // streams consecutive scans alternate over (set per search from the launch size)
    int scan_nstreams_forced = 0;           // tuning.scan_streams
    // uvaia_gpu_db_rederive: chunks of tiles rebuilt on their own stream; a scan waits for the chunks its slice touches
    struct DeriveChunk { long long t0, t1; Event done; };
    Stream derive_streams[3];               // the chunks of a rebuild alternate over the first derive_nstreams
    int derive_nstreams = 3; bool derive_forced = false;   // (forced: tuning.rederive_streams was given)
    std::vector<DeriveChunk> derive_chunks;
    Event derive_fence[4];
    size_t derive_pending = 0;          // chunks of the last rederive a scan may still have to wait for
    // What a rebuild has to queue behind: planes_busy[i] = work that reads or writes the derived planes (a column-compressed scan, a replay,
    // an append's derive) was issued on the stream since the host last waited for it -- [0] `stream` (the masked replay stream is spliced into
    // its order), [1..3] scan_streams; planes_ev[i] = an event the search recorded on that stream behind the last such work (a slice's
    // scan_done / replay_done), null where there is none and the rebuild records one of its own (planes_touch / planes_fenced / planes_idle)
    bool planes_busy[4] = {}; hipEvent_t planes_ev[4] = {};
    Stream rep_stream; Event rep_ev[2];     // replay_cus: the stream masked to them, and the events that splice its kernels into `stream`'s order
    Event order_ev[16]; unsigned order_rr = 0;   // uvaia_gpu_wait_stream: ordering against a caller-owned stream
    Event mark_ev[8][3]; bool mark_set[8][3] = {}; // uvaia_gpu_mark
  } st;
  SliceBuf slice[NBUF];                   // the counter buffers; the push path (run_batch) works in slice[0]
  bool use_ext = false;                   // the scan leaves the extras and replay3_kernel runs (default mode: packed-plane scan, or the column-compressed one up to 128 queries)
  size_t subslice = 25088;                // resident search: pools are cut into slices of about this size (exact: see search_resident).  (32 768 until round 4: at config[1]
                                          // four slices of 25 024 references instead of three of 33 334 cost 9 % more scan time -- a launch carries about 70 us of ramp and
                                          // tail -- and still end 4 % sooner: the first replay starts earlier, the last one is shorter)
  bool subslice_forced = false;           // the length was given (tests): taken as it is
  int first_slice_pct = -1;               // a pool's first slice is this share of an equal one, 0 = equal slices (tuning.scan_streams = 100 + p sets p; 199 = equal slices);
                                          // -1 = the library's choice: equal slices where replay2_lean_kernel runs, 70 elsewhere (see plan_subslices)
  int nq = 0, nq_pad = 0, nchar = 0, W = 0, W4 = 0, P = 4, NQ = 6, acgt = 0, k = 2, qt = 16, n_idx_c = 0, n_idx_m = 0;
  size_t trim = 0;
  size_t max_pool = 0, pool_pad = 0;
  int scan_variant = 2;          // 2 = column-compressed scan3_kernel (default above 32 queries); 0 = scan2_*_kernel over the packed planes
  int derive_waves = 0;          // tuning.derive_waves: 4, 8 or 16 waves per tile for every launch of it (0: derive_rows' caller decides)
  int act_q0 = 0, act_q1 = 0;    // active query range of the resident/slice paths (query shards across GPUs); whole set by default
  bool serial = false;           // tuning.serial: no scan/replay overlap (to time the kernels in isolation)
  int replay_lq = -1;            // replay caches the query's planes in LDS (22 KB per block): -1 = only with few queries (see open)
  int replay_prio = 1;           // replay waves raise their issue priority
  int replay_half = 32;          // tiles per staging buffer of replay3_kernel (32, 16 or 8: its LDS decides how many of its blocks share a compute unit)
  int replay_cus = 0;            // compute units set aside for the replay kernels of the resident search (0: none, the streams share the chip by priority): st.rep_stream
  int scan_R = 2;                // reference tiles per wave of scan3_kernel (the item stream is built for it)
  int scan_NW = 8;               // waves per block of scan3_kernel = shares a super-tile's records are cut into
  bool fullscan = false;         // four-counter scan + the replay over it (alignments above 49 000 columns; tuning.scan = UVAIA_GPU_SCAN_WIDE)
  // ---- query-side tables
  struct QueryTables {
    DevBuf<uint32_t> d_qp;       // [nq_pad][W4][4][NQ]   full-information query planes
    DevBuf<uint32_t> d_qp2;      // [nq_pad][W4][4][4]    (lo, hi, isACGT, valid) for the two-counter scan (default mode)
    // column-compressed scan: classes of the alignment columns for this query set, compressed/dirty query planes, derived reference planes
    DevBuf<uint32_t> d_cls;      // [W4*4][4]  cL, cH, constMask, polyMask
    DevBuf<uint32_t> d_qpl;      // [nq_pad][NP4][L,H,I,-][4]   compressed polymorphic columns of the queries
    DevBuf<uint32_t> d_stream;   // per query tile: the dirty-word item stream of scan3_kernel (layout: see the kernel)
    DevBuf<uint32_t> d_sdir;     // [nq_pad/64][16] per super-tile and wave: {first dword, number} of its group records and of its rare records
    int NP = 0, NP4 = 0;         // polymorphic columns counted densely
    int NR = 0, NR4 = 0, rare_max = -1;   // "rare" columns: all but <= rare_max queries carry the same base; sparse (items), groups follow the dense ones
    DevBuf<uint32_t> d_rmask;    // [W4*4] mask of the rare columns
    DevBuf<int> d_split;         // derive_all_kernel: w4 range and first gathered bit of each of its waves, a section per block width (build_derive_split)
    DevBuf<uint32_t> d_qrare;    // [nq][NR4*4][lo, hi, isACGT] the queries on the rare columns (--acgt: dist_unique of admitted pairs)
    int need_e_groups = 0, need_v_groups = 0, need_g_groups = 0, need_r_groups = 0;   // word groups whose E / V plane some query tile has to read (for the byte accounting)
    DevBuf<int> d_amb_q;         // [nq][AMB_STRIDE] ambiguity-word lists of the queries
    struct { const void *p; size_t n; } qtab[10] = {};   // the query-side tables as uvaia_gpu_export_query_table numbers them (device pointer, bytes)
    DevBuf<uint32_t> d_cp;       // consensus restricted to idx_c, one row [W4][4][NQ]
    DevBuf<uint32_t> d_cpm;      // consensus restricted to idx_m (radius search)
    DevBuf<uint32_t> d_qpoly;    // queries restricted to idx (radius search, redundancy test), [nq_pad][W4][4][NQ]: d_qp masked by d_pmask, built by the first call that needs it
    DevBuf<uint32_t> d_pmask;    // [W4*4] mask of the polymorphic query columns (query->idx)
  } tab;
  // ---- search state
  struct SearchState {
    DevBuf<int> d_heap, d_n, d_T, d_snap, d_err;   // heaps, item counts, tolerances, the batch snapshot; the bad-byte flag of pack_refs_kernel
    DevBuf<int4> d_cnt;          // [nq_pad][pool_pad] four-counter scan output (made by the first call that needs it)
    DevBuf<int4> d_rt, d_tr;     // [pool_pad]
    DevBuf<uint8_t> d_entered;   // [pool_pad] (push) or [db_cap] (resident)
    size_t entered_clean = 0;    // leading bytes of d_entered that uvaia_gpu_reset cleared with no replay issued since (a search that follows need not clear them again)
  } state;
  // ---- radius search
  struct Ball {
    DevBuf<int> d_mindist, d_list, d_cdist, d_n;   // results, the references that go on to the queries
    DevBuf<uint4> d_tiles; unsigned long long asked = 0;
    bool fused = true; DevBuf<uint4> d_ga;   // stage 1 gathers every reference's columns of query->idx itself (tuning.ball_gather)
    Event ev[4]; double ms[3] = {0., 0., 0.};   // per-kernel time of the radius search (host_ball.inc)
    DevBuf<int> d_idx_cols; int n_idx = 0, NG4 = 0;       // query->idx (the polymorphic query columns) and the word groups they fill once gathered
    std::vector<int> idx_cols; DevBuf<uint32_t> d_masks; int NH4 = 0;   // their order in the gathered words: masks [W4][hot 4 | others 4], hot word groups (ensure_qgather)
    DevBuf<uint32_t> d_qg;                                // the queries on those columns (kernels_ball.inc), built by the first radius search
    DevBuf<unsigned long long> d_key;                     // per listed reference: first query that ends the reference's loop (query << 32 | distance)
    // radius search over packed tiles (uvaia_gpu_ball_packed): the four IUPAC planes of the last batch stay here for uvaia_gpu_unpack_rows
    DevBuf<uint4> d_pk; int pk_n = 0;                     // [pool_pad / 64] tiles; references of the last batch (0: none)
    DevBuf<uint8_t> d_rows;                               // text of the selected references, rows of a multiple of 16 bytes (unpack_rows_from: this and the loaded window's)
    DevBuf<int> d_row_idx;
  } ball;
  // ---- rows handed in by device pointer (host_rows.inc): the selection, per row {valid sites, exception records} + flag, record offsets, records
  struct Rows {
    DevBuf<int> d_sel, d_cnt; DevBuf<unsigned long long> d_off; DevBuf<uint2> d_exc;
    std::vector<int> host; std::vector<uint2> exc_host;
    uint32_t run_cut = 0xFFFFFFu;                         // longest exception run of a record (uvaia_gpu_rows_set_run_cut)
    std::vector<Event> evs; double ms[3] = {0., 0., 0.};  // per-kernel time of census, gather, exception fill
  } rows;
  // ---- text row store (host_text.inc): the cleaned text of the references a command appended from device memory, kept as text next to the
  // resident database so that those that enter a heap can be written out; rows of nchar rounded up to 16 bytes, 16-byte aligned
  struct Text {
    DevBuf<uint8_t> d_store, d_out;                       // cap rows of the store; the gathered rows of one round of uvaia_gpu_text_rows
    DevBuf<int> d_idx;
    size_t cap = 0, n = 0;
    Event ev[4]; double ms[2] = {0., 0.};                 // device time of the gathers in, of the gathers out
  } text;
  // ---- windowed search over a packed database larger than device memory (host_window.inc): two staging slots of whole file tiles filled by a copy
  // stream of their own, and (--acgt) the four-plane image of the window loaded last, which the text is decoded from
  struct Window {
    Stream copy_stream;
    struct StageSlot { DevBuf<uint4> planes; DevBuf<int> nonn, side; int n_tiles = 0; Event copied, read; bool read_recorded = false; };
    StageSlot stage[2];          // (the tiles both hold room for: stage_tiles)
    DevBuf<int> d_sel;
    DevBuf<uint4> d_four; int n = 0;      // n: references of the window loaded last (0: none)
    Event ev[5]; double ms[3] = {0., 0., 0.};            // device time of selection, import + derive, decode
    Event slot_ev[2]; double slot_ms = 0.;               // device time of the decode straight out of a slot (uvaia_gpu_db_stage_unpack_rows)
    // uvaia_gpu_db_stage_compact_at: what a compact piece is expanded from -- the base row, the piece's index entries, heads and literals -- on
    // the copy stream's order, so one set serves both slots; device time of the expansion and of the side-row pass
    struct Compact { DevBuf<uint4> base; DevBuf<unsigned long long> hidx, lidx; DevBuf<uint32_t> heads, lits; Event ev[3]; bool timed = false; double ms[2] = {0., 0.}; } compact;
  } win;
  // ---- reference shards (uvaia_gpu_db_set_shard): the stream is dealt in pieces of pt tiles, piece p belongs to rank p % world; the packed
  // planes of ALL references are resident (the replay reads them), the planes derived for the query set only for the owned pieces
  struct Shard {
    int rank = 0, world = 1; long long pt = 0;
    const uint4 *peer_db[64] = {}; const int *peer_amb[64] = {};      // packed planes and side rows of every rank's pieces, as this process can address them
    void *ipc_opened[64][2] = {};                                    // mappings opened by uvaia_gpu_shard_ipc_open (closed with the context)
  } shard;
  // ---- batch buffers
  TileStore batch;               // the current batch (ensure_batch_buffers)
  DevBuf<uint8_t> d_stage;       // device staging for raw characters (2 x PACK_CHUNK rows)
  PinnedBuf h_stage;             // pinned host staging (2 x PACK_CHUNK rows)
  Event stage_free[2]; bool stage_busy[2] = {};
  size_t pitch = 0;
  // ---- resident database
  TileStore db;
  size_t db_cap = 0, db_n = 0, db_local_tiles = 0;   // (db_n counts the stream; a context of a reference shard keeps db_local_tiles tiles of it)
  unsigned long long db_gen = 0;                     // counts the calls that changed the resident database (appends, loads, skips, clears, dropped tiles)
  // ---- resident tiles written in the compact form (host_encode.inc): the base, per lane the counts and the offsets they sum to, the records;
  // the plan uvaia_gpu_db_encode_compact leaves for uvaia_gpu_db_encoded_records holds while db_gen is the one it was made at
  struct Encode {
    DevBuf<uint4> base, lits; DevBuf<uint32_t> cnt_h, cnt_l, heads; DevBuf<unsigned long long> hidx, lidx;
    Event ev[4]; double ms[2] = {0., 0.};              // device time of count + prefix, of emit
    bool plan = false; size_t first_tile = 0, n_tiles = 0; unsigned long long db_gen = 0, n_heads = 0, n_lits = 0;
  } enc;
  // ---- all pairs of the resident database (host_pairs.inc): the row operand records of a band, the counters of one launch, the list of one
  // launch and its length; everything is sized by the rectangle of a launch
  struct Pairs {
    DevBuf<uint32_t> d_rec; DevBuf<int> d_out; DevBuf<uvaia_gpu_pair> d_list; DevBuf<unsigned long long> d_count;
    Event ev[2]; double ms[3] = {0., 0., 0.};          // device time of the row operands, the dense kernels, the threshold kernels (+ the host's sort)
    // single-linkage clusters (uvaia_gpu_db_link_*): the forest, one dword per reference resident at `begin`, the labels read off it, what
    // `begin` was given, and the database it was given for (links are refused once db_gen has moved on)
    DevBuf<uint32_t> d_parent, d_labels; double link_ms = 0.;      // device time of the link and label kernels
    struct { bool begun = false; unsigned long long db_gen = 0; size_t n = 0, trim = 0; int metric = 0, max_dist = 0, min_compared = 0; } link;
    // closest reference of another component (uvaia_gpu_db_near_*, uvaia_gpu_db_mst): 12 bytes per reference resident at `begin` -- the
    // packed keys and the components -- the two counters of tile pairs, and the host's copy of the components (it decides which launches
    // are skipped whole)
    DevBuf<unsigned long long> d_best, d_near_stats; DevBuf<uint32_t> d_comp; double near_ms = 0.;  // device time of the near kernels
    unsigned long long near_tiles[2] = {0, 0};         // tile pairs walked, skipped since the last reset
    std::vector<uint32_t> h_comp;
    struct { bool begun = false; unsigned long long db_gen = 0; size_t n = 0, trim = 0; int metric = 0, min_compared = 0; } near;
  } pairs;
  // last batch (introspection)
  struct { const TileStore *store = nullptr; long long tile_first = 0; int n_tiles = 0, n = 0, rbegin = 0, ppad = 0; const int4 *rt = nullptr; } last;
  // ---- statistics
  struct Stats {
    DevBuf<unsigned long long> d_stats;           // admissions, on-demand evaluations, dense fallbacks, tiles opened (replay3_kernel)
    std::vector<ScanEvt> evts;
    std::vector<Event> ev_pool;         // timing events of earlier launches, reused (creating and destroying a pair per launch was 50-100 us of host time per step)
    double scan_ms = 0, scan_bytes = 0; long long scan_launches = 0;
    bool profile = true;
  } stats;
  std::string err;
};

namespace {

int fail(uvaia_gpu_ctx *c, int code, const char *fmt, ...)
{
  char buf[512];
  va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
  if (c) c->err = buf; else g_open_error = buf;
  return code;
}

// Reference shards: the per-reference arrays of the resident database -- packed planes, side rows, counts, derived planes -- hold the
// context's OWN pieces only, numbered densely ("local" tiles: dtile_of); positions in the stream, ordinals and the dump flags stay
// global.  owns_tile: does this context keep (global) tile t;  dtile_of: its local number on the context that keeps it (the same formula
// on every rank: a replaying rank uses it to find a reference in the memory of the rank that scanned it).
inline bool owns_tile(const uvaia_gpu_ctx *c, long long t) { return c->shard.world == 1 || (t / c->shard.pt) % c->shard.world == c->shard.rank; }
inline long long dtile_of(const uvaia_gpu_ctx *c, long long t)
{ return c->shard.world == 1 ? t : (t / (c->shard.pt * c->shard.world)) * c->shard.pt + t % c->shard.pt; }
// the owned parts of the global tiles [gt0, gt1): f(global first tile, local first tile, number of tiles) per part inside one piece
template <class F> inline int for_owned_tiles(const uvaia_gpu_ctx *c, long long gt0, long long gt1, F f)
{
  if (c->shard.world == 1) return gt1 > gt0 ? f(gt0, gt0, gt1 - gt0) : 0;
  for (long long a = gt0; a < gt1;) {
    const long long b = std::min(gt1, (a / c->shard.pt + 1) * c->shard.pt);
    if (owns_tile(c, a)) { const int rc = f(a, dtile_of(c, a), b - a); if (rc) return rc; }
    a = b;
  }
  return 0;
}
inline size_t derived_tiles(const uvaia_gpu_ctx *c, size_t tiles)
{ return c->shard.world == 1 ? tiles : (size_t)((tiles + (size_t)(c->shard.pt * c->shard.world) - 1) / (size_t)(c->shard.pt * c->shard.world)) * (size_t)c->shard.pt; }

// IUPAC code table: 1..15 = nucleotide set (A=1 C=2 G=4 T=8), 0 = invalid site (N X - ? O .), 0xFF = refused
void fill_code_table(uint8_t *t)
{
  memset(t, 0xFF, 256);
  const char *inv = "NnXx-?Oo.";                      // src/utils.c:263
  for (const char *p = inv; *p; p++) t[(unsigned char)*p] = 0;
  static const struct { char c; uint8_t m; } iu[] = {
    {'A',1},{'C',2},{'G',4},{'T',8},{'M',3},{'R',5},{'W',9},{'S',6},{'Y',10},{'K',12},{'V',7},{'H',11},{'D',13},{'B',14}};
  for (auto &e : iu) { t[(unsigned char)e.c] = e.m; t[(unsigned char)(e.c + 32)] = e.m; }
}

}  // namespace
