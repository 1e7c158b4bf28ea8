// host_pairs.inc -- part of uvaia_gpu.hip (included there, not a translation unit of its own): all pairs of the resident database against each other:
// the checks, the cut of a rectangle into launches, the copies back, the list of the pairs within a distance, and the single-linkage
// clusters within a distance (a forest on the device: begin, link, labels), every reference's closest reference of another component
// (begin, components, near, fetch) and the Boruvka rounds of the minimum spanning forest around it.

namespace {

// One launch covers at most this rectangle: the counters of a launch (32 MiB as distances, 160 MiB as five counters), its list and the row
// records of a band (a few tens of MiB at 30 000 columns) are all the working memory, whatever the database holds.
constexpr size_t PAIRS_LAUNCH_ROWS = 1024, PAIRS_LAUNCH_COLS = 8192;
constexpr int PAIRS_SNP_RT = 32, PAIRS_SNP_RT_ALT = 64;   // rows per wave of pairs_snp_kernel (DESIGN.md 4.12 has both heights measured)

// what both entries refuse before anything is launched
int pairs_check(uvaia_gpu_ctx *c, size_t row0, size_t n_rows, size_t col0, size_t n_cols, size_t trim)
{
  if (c->acgt) return fail(c, UVAIA_GPU_ESTATE, "pair counters are taken over the four IUPAC planes: use a default-mode context");
  if (c->shard.world > 1) return fail(c, UVAIA_GPU_ESTATE, "a context of a reference shard holds its own pieces only: pairs are counted in a plain context");
  if (row0 > c->db_n || n_rows > c->db_n - row0) return fail(c, UVAIA_GPU_EINVAL, "rows %zu..%zu lie outside the database of %zu references", row0, row0 + n_rows, c->db_n);
  if (col0 > c->db_n || n_cols > c->db_n - col0) return fail(c, UVAIA_GPU_EINVAL, "columns %zu..%zu lie outside the database of %zu references", col0, col0 + n_cols, c->db_n);
  if (trim > (size_t)c->nchar || 2 * trim > (size_t)c->nchar) return fail(c, UVAIA_GPU_EINVAL, "trim %zu on both sides leaves nothing of %d sites", trim, c->nchar);
  return 0;
}

// nothing of this context may still be reading or writing the resident planes (searches in flight, a rebuild of the derived planes shares the streams)
int pairs_wait(uvaia_gpu_ctx *c)
{
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = settle_derive(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->st.stream));
  return sync_scan_streams(c);
}

int pairs_add_ms(uvaia_gpu_ctx *c, int which)
{ // (the stream has been waited for)
  float ms = 0;
  HIPCHK(c, hipEventElapsedTime(&ms, c->pairs.ev[0], c->pairs.ev[1]));
  c->pairs.ms[which] += ms;
  return 0;
}

// the row operand records of rows [row0, row0 + n) (n <= PAIRS_LAUNCH_ROWS), padded to whole blocks of 64 rows; waits for them (the time is read)
template <int D> int pairs_build_rows(uvaia_gpu_ctx *c, size_t row0, size_t n, size_t trim)
{
  const size_t rows_pad = (n + 63) / 64 * 64;
  if (int rc = c->pairs.d_rec.reserve(c, PAIRS_LAUNCH_ROWS * (size_t)c->W4 * PAIRS_CNT_DW)) return rc;     // one size for both forms: no regrowth between calls
  HIPCHK(c, hipEventRecord(c->pairs.ev[0], c->st.stream));
  hipLaunchKernelGGL((pairs_rows_kernel<D>), dim3((unsigned)(rows_pad / 64), (unsigned)((c->W4 + 3) / 4)), dim3(256), 0, c->st.stream,
                     (const uint4 *)c->db.planes, c->W4, (long long)row0, (int)n, (int)trim, (int)((size_t)c->nchar - trim), c->pairs.d_rec.p);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(c->pairs.ev[1], c->st.stream));
  HIPCHK(c, hipStreamSynchronize(c->st.stream));
  return pairs_add_ms(c, 0);
}

inline unsigned pairs_grid(size_t n_rows, int rt, int n_ctiles) { return (unsigned)((n_rows + rt - 1) / rt) * (unsigned)((n_ctiles + 3) / 4); }

// a clustering is open, and over the database as it is now (the forest has one node per reference resident at `begin`)
int link_state(uvaia_gpu_ctx *c)
{
  const auto &k = c->pairs.link;
  if (!k.begun) return fail(c, UVAIA_GPU_ESTATE, "no clustering is open: call uvaia_gpu_db_link_begin first");
  if (k.db_gen != c->db_gen || k.n != c->db_n) return fail(c, UVAIA_GPU_ESTATE, "the database changed since uvaia_gpu_db_link_begin: begin again");
  return 0;
}

// the keys are open, and over the database as it is now (best[] and comp[] have one element per reference resident at `begin`)
int near_state(uvaia_gpu_ctx *c)
{
  const auto &k = c->pairs.near;
  if (!k.begun) return fail(c, UVAIA_GPU_ESTATE, "no nearest-reference pass is open: call uvaia_gpu_db_near_begin first");
  if (k.db_gen != c->db_gen || k.n != c->db_n) return fail(c, UVAIA_GPU_ESTATE, "the database changed since uvaia_gpu_db_near_begin: begin again");
  return 0;
}

}  // namespace

extern "C" {

int uvaia_gpu_db_pairs(uvaia_gpu_ctx *c, size_t row0, size_t n_rows, size_t col0, size_t n_cols, size_t trim, int what, int32_t *out, size_t ld)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (what != UVAIA_GPU_PAIRS_SNP && what != UVAIA_GPU_PAIRS_COUNTS && what != UVAIA_GPU_PAIRS_SNP_ALT) return fail(c, UVAIA_GPU_EINVAL, "unknown kind of pair output %d", what);
  if (int rc = pairs_check(c, row0, n_rows, col0, n_cols, trim)) return rc;
  if (!n_rows || !n_cols) return 0;
  if (!out || ld < n_cols) return fail(c, UVAIA_GPU_EINVAL, "NULL output or a leading dimension below the %zu columns", n_cols);
  if (int rc = pairs_wait(c)) return rc;
  if (int rc = c->pairs.ev[0].make(c)) return rc;
  if (int rc = c->pairs.ev[1].make(c)) return rc;
  const bool counts = what == UVAIA_GPU_PAIRS_COUNTS;
  const size_t per = counts ? UVAIA_GPU_PAIR_NCOUNT : 1;
  const int rt = counts ? PAIRS_CNT_RT : what == UVAIA_GPU_PAIRS_SNP ? PAIRS_SNP_RT : PAIRS_SNP_RT_ALT;
  if (int rc = c->pairs.d_out.reserve(c, std::min(n_rows, PAIRS_LAUNCH_ROWS) * std::min(n_cols, PAIRS_LAUNCH_COLS) * per)) return rc;
  const uint4 *db = c->db.planes;
  for (size_t rb = 0; rb < n_rows; rb += PAIRS_LAUNCH_ROWS) {
    const size_t nr = std::min(PAIRS_LAUNCH_ROWS, n_rows - rb);
    if (int rc = counts ? pairs_build_rows<PAIRS_CNT_DW>(c, row0 + rb, nr, trim) : pairs_build_rows<PAIRS_SNP_DW>(c, row0 + rb, nr, trim)) return rc;
    for (size_t cb = 0; cb < n_cols; cb += PAIRS_LAUNCH_COLS) {
      const size_t nc = std::min(PAIRS_LAUNCH_COLS, n_cols - cb), c0 = col0 + cb;
      const long long ct0 = (long long)(c0 / 64);
      const int n_ct = (int)((c0 + nc - 1) / 64 - c0 / 64 + 1), n_rt = (int)((nr + rt - 1) / rt);
      const dim3 grid(pairs_grid(nr, rt, n_ct));
      HIPCHK(c, hipEventRecord(c->pairs.ev[0], c->st.stream));
      if (counts)
        hipLaunchKernelGGL((pairs_counts_kernel<PAIRS_DENSE>), grid, dim3(256), 0, c->st.stream, db, c->W4, (const uint32_t *)c->pairs.d_rec.p, (long long)(row0 + rb), (int)nr, n_rt, ct0, n_ct,
                           (long long)c0, (int)nc, c->pairs.d_out.p, nc, 0, 0, 0, (uvaia_gpu_pair *)nullptr, 0ull, (unsigned long long *)nullptr, 0, (uint32_t *)nullptr, (unsigned long long *)nullptr);
      else if (rt == 32)
        hipLaunchKernelGGL((pairs_snp_kernel<32>), grid, dim3(256), 0, c->st.stream, db, c->W4, (const uint32_t *)c->pairs.d_rec.p, (int)nr, n_rt, ct0, n_ct, (long long)c0, (int)nc, c->pairs.d_out.p, nc);
      else
        hipLaunchKernelGGL((pairs_snp_kernel<64>), grid, dim3(256), 0, c->st.stream, db, c->W4, (const uint32_t *)c->pairs.d_rec.p, (int)nr, n_rt, ct0, n_ct, (long long)c0, (int)nc, c->pairs.d_out.p, nc);
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, hipEventRecord(c->pairs.ev[1], c->st.stream));
      HIPCHK(c, hipMemcpy2DAsync(out + (rb * ld + cb) * per, ld * per * sizeof(int32_t), c->pairs.d_out.p, nc * per * sizeof(int32_t), nc * per * sizeof(int32_t), nr,
                                 hipMemcpyDeviceToHost, c->st.stream));
      HIPCHK(c, hipStreamSynchronize(c->st.stream));
      if (int rc = pairs_add_ms(c, 1)) return rc;
    }
  }
  return 0;
}

int uvaia_gpu_db_pairs_within(uvaia_gpu_ctx *c, size_t row0, size_t n_rows, size_t col0, size_t n_cols, size_t trim, int metric, int max_dist, int upper,
                              uvaia_gpu_pair *out, size_t cap, unsigned long long *n_found)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (metric != UVAIA_GPU_DIST_SNP && metric != UVAIA_GPU_DIST_UVAIA) return fail(c, UVAIA_GPU_EINVAL, "unknown metric %d", metric);
  if (max_dist < 0) return fail(c, UVAIA_GPU_EINVAL, "negative distance %d", max_dist);
  if (!n_found || (cap && !out)) return fail(c, UVAIA_GPU_EINVAL, "NULL list or count");
  if (int rc = pairs_check(c, row0, n_rows, col0, n_cols, trim)) return rc;
  *n_found = 0;
  if (!n_rows || !n_cols) return 0;
  if (int rc = pairs_wait(c)) return rc;
  if (int rc = c->pairs.ev[0].make(c)) return rc;
  if (int rc = c->pairs.ev[1].make(c)) return rc;
  const size_t launch_pairs = std::min(n_rows, PAIRS_LAUNCH_ROWS) * std::min(n_cols, PAIRS_LAUNCH_COLS);
  if (int rc = c->pairs.d_list.reserve(c, std::max<size_t>(1, std::min(cap, launch_pairs)))) return rc;
  if (int rc = c->pairs.d_count.reserve(c, 1)) return rc;
  const uint4 *db = c->db.planes;
  unsigned long long found = 0;
  for (size_t rb = 0; rb < n_rows; rb += PAIRS_LAUNCH_ROWS) {
    const size_t nr = std::min(PAIRS_LAUNCH_ROWS, n_rows - rb);
    if (int rc = pairs_build_rows<PAIRS_CNT_DW>(c, row0 + rb, nr, trim)) return rc;
    for (size_t cb = 0; cb < n_cols; cb += PAIRS_LAUNCH_COLS) {
      const size_t nc = std::min(PAIRS_LAUNCH_COLS, n_cols - cb), c0 = col0 + cb;
      if (upper && c0 + nc <= row0 + rb + 1) continue;           // no pair of this launch has row < col
      const long long ct0 = (long long)(c0 / 64);
      const int n_ct = (int)((c0 + nc - 1) / 64 - c0 / 64 + 1), n_rt = (int)((nr + PAIRS_CNT_RT - 1) / PAIRS_CNT_RT);
      // what of the caller's list is still free bounds the stores of this launch (never more than the launch has pairs: the device list's size)
      const unsigned long long room = found < cap ? std::min<unsigned long long>(cap - found, nr * nc) : 0ull;
      HIPCHK(c, hipMemsetAsync(c->pairs.d_count.p, 0, sizeof(unsigned long long), c->st.stream));
      HIPCHK(c, hipEventRecord(c->pairs.ev[0], c->st.stream));
      hipLaunchKernelGGL((pairs_counts_kernel<PAIRS_LIST>), dim3(pairs_grid(nr, PAIRS_CNT_RT, n_ct)), dim3(256), 0, c->st.stream, db, c->W4, (const uint32_t *)c->pairs.d_rec.p,
                         (long long)(row0 + rb), (int)nr, n_rt, ct0, n_ct, (long long)c0, (int)nc, (int *)nullptr, (size_t)0, metric, max_dist, upper ? 1 : 0,
                         c->pairs.d_list.p, room, c->pairs.d_count.p, 0, (uint32_t *)nullptr, (unsigned long long *)nullptr);
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, hipEventRecord(c->pairs.ev[1], c->st.stream));
      unsigned long long n_here = 0;
      HIPCHK(c, hipMemcpyAsync(&n_here, c->pairs.d_count.p, sizeof n_here, hipMemcpyDeviceToHost, c->st.stream));
      HIPCHK(c, hipStreamSynchronize(c->st.stream));
      if (int rc = pairs_add_ms(c, 2)) return rc;
      const unsigned long long take = std::min(n_here, room);
      if (take) HIPCHK(c, hipMemcpy(out + found, c->pairs.d_list.p, (size_t)take * sizeof(uvaia_gpu_pair), hipMemcpyDeviceToHost));
      found += n_here;
    }
  }
  *n_found = found;
  if (found <= cap && found > 1) {
    const auto t0 = std::chrono::steady_clock::now();
    std::sort(out, out + found, [](const uvaia_gpu_pair &a, const uvaia_gpu_pair &b) { return a.row != b.row ? a.row < b.row : a.col < b.col; });
    c->pairs.ms[2] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  return 0;
}

void uvaia_gpu_pairs_ms(uvaia_gpu_ctx *c, double out[3], int reset)
{
  if (!c) return;
  if (out) for (int i = 0; i < 3; i++) out[i] = c->pairs.ms[i];
  if (reset) c->pairs.ms[0] = c->pairs.ms[1] = c->pairs.ms[2] = 0.;
}

// ---- single-linkage clusters: the pairs within a distance united in a forest on the device
int uvaia_gpu_db_link_begin(uvaia_gpu_ctx *c, size_t trim, int metric, int max_dist, int min_compared)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (metric != UVAIA_GPU_DIST_SNP && metric != UVAIA_GPU_DIST_UVAIA) return fail(c, UVAIA_GPU_EINVAL, "unknown metric %d", metric);
  if (max_dist < 0) return fail(c, UVAIA_GPU_EINVAL, "negative distance %d", max_dist);
  if (min_compared < 0) return fail(c, UVAIA_GPU_EINVAL, "negative floor of compared sites %d", min_compared);
  if (int rc = pairs_check(c, 0, c->db_n, 0, c->db_n, trim)) return rc;
  if (c->db_n > 0xFFFFFFFFull) return fail(c, UVAIA_GPU_EINVAL, "cluster labels are 32-bit database positions: %zu references are too many", c->db_n);
  auto &k = c->pairs.link;
  k.begun = false;
  if (int rc = pairs_wait(c)) return rc;
  if (int rc = c->pairs.d_parent.reserve(c, std::max<size_t>(1, c->db_n))) return rc;
  if (c->db_n) {
    hipLaunchKernelGGL(pairs_link_init_kernel, dim3((unsigned)((c->db_n + 255) / 256)), dim3(256), 0, c->st.stream, c->pairs.d_parent.p, (uint32_t)c->db_n);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->st.stream));
  }
  k.begun = true; k.db_gen = c->db_gen; k.n = c->db_n; k.trim = trim; k.metric = metric; k.max_dist = max_dist; k.min_compared = min_compared;
  return 0;
}

int uvaia_gpu_db_link(uvaia_gpu_ctx *c, size_t row0, size_t n_rows, size_t col0, size_t n_cols, unsigned long long *n_links)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (int rc = link_state(c)) return rc;
  if (!n_links) return fail(c, UVAIA_GPU_EINVAL, "NULL count of links");
  const auto &k = c->pairs.link;
  if (int rc = pairs_check(c, row0, n_rows, col0, n_cols, k.trim)) return rc;
  if (!n_rows || !n_cols) return 0;
  if (int rc = pairs_wait(c)) return rc;
  if (int rc = c->pairs.ev[0].make(c)) return rc;
  if (int rc = c->pairs.ev[1].make(c)) return rc;
  if (int rc = c->pairs.d_count.reserve(c, 1)) return rc;
  const bool snp = k.metric == UVAIA_GPU_DIST_SNP;
  const int rt = snp ? PAIRS_SNP_RT : PAIRS_CNT_RT;
  const uint4 *db = c->db.planes;
  const uint32_t *rec = nullptr;
  HIPCHK(c, hipMemsetAsync(c->pairs.d_count.p, 0, sizeof(unsigned long long), c->st.stream));      // one count for the launches of this call
  for (size_t rb = 0; rb < n_rows; rb += PAIRS_LAUNCH_ROWS) {
    const size_t nr = std::min(PAIRS_LAUNCH_ROWS, n_rows - rb);
    if (col0 + n_cols <= row0 + rb + 1) break;                   // this band and every later one lie at or below the diagonal
    if (int rc = snp ? pairs_build_rows<PAIRS_SNP_DW>(c, row0 + rb, nr, k.trim) : pairs_build_rows<PAIRS_CNT_DW>(c, row0 + rb, nr, k.trim)) return rc;
    rec = c->pairs.d_rec.p;
    for (size_t cb = 0; cb < n_cols; cb += PAIRS_LAUNCH_COLS) {
      const size_t nc = std::min(PAIRS_LAUNCH_COLS, n_cols - cb), c0 = col0 + cb;
      if (c0 + nc <= row0 + rb + 1) continue;                    // no pair of this launch has row < col
      const long long ct0 = (long long)(c0 / 64);
      const int n_ct = (int)((c0 + nc - 1) / 64 - c0 / 64 + 1), n_rt = (int)((nr + rt - 1) / rt);
      const dim3 grid(pairs_grid(nr, rt, n_ct));
      HIPCHK(c, hipEventRecord(c->pairs.ev[0], c->st.stream));
      if (!snp)
        hipLaunchKernelGGL((pairs_counts_kernel<PAIRS_LINK>), grid, dim3(256), 0, c->st.stream, db, c->W4, rec, (long long)(row0 + rb), (int)nr, n_rt, ct0, n_ct, (long long)c0, (int)nc,
                           (int *)nullptr, (size_t)0, k.metric, k.max_dist, 1, (uvaia_gpu_pair *)nullptr, 0ull, c->pairs.d_count.p, k.min_compared, c->pairs.d_parent.p, (unsigned long long *)nullptr);
      else if (k.min_compared > 0)
        hipLaunchKernelGGL((pairs_link_snp_kernel<true>), grid, dim3(256), 0, c->st.stream, db, c->W4, rec, (long long)(row0 + rb), (int)nr, n_rt, ct0, n_ct, (long long)c0, (int)nc,
                           k.max_dist, k.min_compared, c->pairs.d_parent.p, c->pairs.d_count.p);
      else
        hipLaunchKernelGGL((pairs_link_snp_kernel<false>), grid, dim3(256), 0, c->st.stream, db, c->W4, rec, (long long)(row0 + rb), (int)nr, n_rt, ct0, n_ct, (long long)c0, (int)nc,
                           k.max_dist, 0, c->pairs.d_parent.p, c->pairs.d_count.p);
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, hipEventRecord(c->pairs.ev[1], c->st.stream));
      HIPCHK(c, hipStreamSynchronize(c->st.stream));             // (the next band's row records overwrite the ones this launch reads)
      float ms = 0;
      HIPCHK(c, hipEventElapsedTime(&ms, c->pairs.ev[0], c->pairs.ev[1]));
      c->pairs.link_ms += ms;
    }
  }
  unsigned long long found = 0;                                  // read in stream order: behind the memset also where every launch was skipped
  HIPCHK(c, hipMemcpyAsync(&found, c->pairs.d_count.p, sizeof found, hipMemcpyDeviceToHost, c->st.stream));
  HIPCHK(c, hipStreamSynchronize(c->st.stream));
  *n_links += found;
  return 0;
}

int uvaia_gpu_db_link_labels(uvaia_gpu_ctx *c, uint32_t *labels)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (int rc = link_state(c)) return rc;
  const size_t n = c->pairs.link.n;
  if (!n) return 0;
  if (!labels) return fail(c, UVAIA_GPU_EINVAL, "NULL labels");
  if (int rc = pairs_wait(c)) return rc;
  if (int rc = c->pairs.ev[0].make(c)) return rc;
  if (int rc = c->pairs.ev[1].make(c)) return rc;
  if (int rc = c->pairs.d_labels.reserve(c, n)) return rc;
  HIPCHK(c, hipEventRecord(c->pairs.ev[0], c->st.stream));
  hipLaunchKernelGGL(pairs_labels_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->st.stream, (const uint32_t *)c->pairs.d_parent.p, (uint32_t)n, c->pairs.d_labels.p);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(c->pairs.ev[1], c->st.stream));
  HIPCHK(c, hipMemcpyAsync(labels, c->pairs.d_labels.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->st.stream));
  HIPCHK(c, hipStreamSynchronize(c->st.stream));
  float ms = 0;
  HIPCHK(c, hipEventElapsedTime(&ms, c->pairs.ev[0], c->pairs.ev[1]));
  c->pairs.link_ms += ms;
  return 0;
}

void uvaia_gpu_link_ms(uvaia_gpu_ctx *c, double *ms, int reset)
{
  if (!c) return;
  if (ms) *ms = c->pairs.link_ms;
  if (reset) c->pairs.link_ms = 0.;
}

// ---- every reference's closest reference of another component, and the minimum spanning forest by Boruvka rounds around it
int uvaia_gpu_db_near_begin(uvaia_gpu_ctx *c, size_t trim, int metric, int min_compared)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (metric != UVAIA_GPU_DIST_SNP && metric != UVAIA_GPU_DIST_UVAIA) return fail(c, UVAIA_GPU_EINVAL, "unknown metric %d", metric);
  if (min_compared < 0) return fail(c, UVAIA_GPU_EINVAL, "negative floor of compared sites %d", min_compared);
  if (int rc = pairs_check(c, 0, c->db_n, 0, c->db_n, trim)) return rc;
  if (c->db_n > 0xFFFFFFFFull) return fail(c, UVAIA_GPU_EINVAL, "the keys hold 32-bit database positions: %zu references are too many", c->db_n);
  auto &k = c->pairs.near;
  k.begun = false;
  if (int rc = pairs_wait(c)) return rc;
  const size_t n = std::max<size_t>(1, c->db_n);
  if (int rc = c->pairs.d_best.reserve(c, n)) return rc;
  if (int rc = c->pairs.d_comp.reserve(c, n)) return rc;
  if (int rc = c->pairs.d_near_stats.reserve(c, 2)) return rc;
  k.begun = true; k.db_gen = c->db_gen; k.n = c->db_n; k.trim = trim; k.metric = metric; k.min_compared = min_compared;
  if (int rc = uvaia_gpu_db_near_components(c, nullptr)) { k.begun = false; return rc; }
  return 0;
}

int uvaia_gpu_db_near_components(uvaia_gpu_ctx *c, const uint32_t *comp)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (int rc = near_state(c)) return rc;
  const size_t n = c->pairs.near.n;
  auto &h = c->pairs.h_comp;
  h.resize(n);
  if (comp) std::copy(comp, comp + n, h.begin());
  else std::iota(h.begin(), h.end(), 0u);
  if (!n) return 0;
  if (int rc = pairs_wait(c)) return rc;
  if (comp) HIPCHK(c, hipMemcpyAsync(c->pairs.d_comp.p, h.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, c->st.stream));
  hipLaunchKernelGGL(pairs_near_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->st.stream, c->pairs.d_best.p, c->pairs.d_comp.p, (uint32_t)n, comp ? 0 : 1);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->st.stream));       // (h_comp may be handed in again; the near kernels read comp[] by plain loads)
  return 0;
}

int uvaia_gpu_db_near(uvaia_gpu_ctx *c, size_t row0, size_t n_rows, size_t col0, size_t n_cols, unsigned long long stats[2])
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (int rc = near_state(c)) return rc;
  const auto &k = c->pairs.near;
  if (int rc = pairs_check(c, row0, n_rows, col0, n_cols, k.trim)) return rc;
  if (!n_rows || !n_cols) return 0;
  if (int rc = pairs_wait(c)) return rc;
  if (int rc = c->pairs.ev[0].make(c)) return rc;
  if (int rc = c->pairs.ev[1].make(c)) return rc;
  const bool snp = k.metric == UVAIA_GPU_DIST_SNP;
  const int rt = snp ? PAIRS_SNP_RT : PAIRS_CNT_RT;
  const uint4 *db = c->db.planes;
  const uint32_t *comp = c->pairs.h_comp.data();
  unsigned long long skipped_whole = 0;
  HIPCHK(c, hipMemsetAsync(c->pairs.d_near_stats.p, 0, 2 * sizeof(unsigned long long), c->st.stream));   // the counters of this call's launches
  for (size_t rb = 0; rb < n_rows; rb += PAIRS_LAUNCH_ROWS) {
    const size_t nr = std::min(PAIRS_LAUNCH_ROWS, n_rows - rb);
    if (col0 + n_cols <= row0 + rb + 1) break;                   // this band and every later one lie at or below the diagonal
    const uint32_t one = comp[row0 + rb];
    const bool rows_one = std::all_of(comp + row0 + rb, comp + row0 + rb + nr, [one](uint32_t x) { return x == one; });
    bool built = false;                                          // the row records are built in front of the band's first launch
    for (size_t cb = 0; cb < n_cols; cb += PAIRS_LAUNCH_COLS) {
      const size_t nc = std::min(PAIRS_LAUNCH_COLS, n_cols - cb), c0 = col0 + cb;
      if (c0 + nc <= row0 + rb + 1) continue;                    // no pair of this launch has row < col
      const long long ct0 = (long long)(c0 / 64);
      const int n_ct = (int)((c0 + nc - 1) / 64 - c0 / 64 + 1), n_rt = (int)((nr + rt - 1) / rt);
      if (rows_one && std::all_of(comp + c0, comp + c0 + nc, [one](uint32_t x) { return x == one; })) {
        skipped_whole += (unsigned long long)n_rt * (unsigned long long)n_ct;      // its rows and columns are one component: no pair of it counts
        continue;
      }
      if (!built) {
        if (int rc = snp ? pairs_build_rows<PAIRS_SNP_DW>(c, row0 + rb, nr, k.trim) : pairs_build_rows<PAIRS_CNT_DW>(c, row0 + rb, nr, k.trim)) return rc;
        built = true;
      }
      const uint32_t *rec = c->pairs.d_rec.p;
      const dim3 grid(pairs_grid(nr, rt, n_ct));
      HIPCHK(c, hipEventRecord(c->pairs.ev[0], c->st.stream));
      if (!snp)
        hipLaunchKernelGGL((pairs_counts_kernel<PAIRS_NEAR>), grid, dim3(256), 0, c->st.stream, db, c->W4, rec, (long long)(row0 + rb), (int)nr, n_rt, ct0, n_ct, (long long)c0, (int)nc,
                           (int *)nullptr, (size_t)0, k.metric, 0, 1, (uvaia_gpu_pair *)nullptr, 0ull, c->pairs.d_near_stats.p, k.min_compared, c->pairs.d_comp.p, c->pairs.d_best.p);
      else if (k.min_compared > 0)
        hipLaunchKernelGGL((pairs_near_snp_kernel<true>), grid, dim3(256), 0, c->st.stream, db, c->W4, rec, (long long)(row0 + rb), (int)nr, n_rt, ct0, n_ct, (long long)c0, (int)nc,
                           k.min_compared, (const uint32_t *)c->pairs.d_comp.p, c->pairs.d_best.p, c->pairs.d_near_stats.p);
      else
        hipLaunchKernelGGL((pairs_near_snp_kernel<false>), grid, dim3(256), 0, c->st.stream, db, c->W4, rec, (long long)(row0 + rb), (int)nr, n_rt, ct0, n_ct, (long long)c0, (int)nc,
                           0, (const uint32_t *)c->pairs.d_comp.p, c->pairs.d_best.p, c->pairs.d_near_stats.p);
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, hipEventRecord(c->pairs.ev[1], c->st.stream));
      HIPCHK(c, hipStreamSynchronize(c->st.stream));             // (the next band's row records overwrite the ones this launch reads)
      float ms = 0;
      HIPCHK(c, hipEventElapsedTime(&ms, c->pairs.ev[0], c->pairs.ev[1]));
      c->pairs.near_ms += ms;
    }
  }
  unsigned long long seen[2] = {0, 0};                           // read in stream order: behind the memset also where every launch was skipped
  HIPCHK(c, hipMemcpyAsync(seen, c->pairs.d_near_stats.p, sizeof seen, hipMemcpyDeviceToHost, c->st.stream));
  HIPCHK(c, hipStreamSynchronize(c->st.stream));
  c->pairs.near_tiles[0] += seen[0]; c->pairs.near_tiles[1] += seen[1] + skipped_whole;
  if (stats) { stats[0] += seen[0]; stats[1] += seen[1] + skipped_whole; }
  return 0;
}

int uvaia_gpu_db_near_fetch(uvaia_gpu_ctx *c, uint64_t *best)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (int rc = near_state(c)) return rc;
  const size_t n = c->pairs.near.n;
  if (!n) return 0;
  if (!best) return fail(c, UVAIA_GPU_EINVAL, "NULL keys");
  if (int rc = pairs_wait(c)) return rc;
  HIPCHK(c, hipMemcpyAsync(best, c->pairs.d_best.p, n * sizeof(uint64_t), hipMemcpyDeviceToHost, c->st.stream));
  HIPCHK(c, hipStreamSynchronize(c->st.stream));
  return 0;
}

// Boruvka: a round gives every reference its closest reference of another component (one pass of the matrix), the host takes every
// component's minimum under the edge order (dist, lo, hi) and unites.  The order is strict and total, so the edges chosen in a round close
// no cycle and all belong to the one minimum spanning forest (DESIGN.md 4.12); a component with no outgoing edge is a finished tree.
int uvaia_gpu_db_mst(uvaia_gpu_ctx *c, size_t trim, int metric, int min_compared, uvaia_gpu_edge *edges, size_t *n_edges, int *n_rounds)
{
  if (!c) return UVAIA_GPU_EINVAL;
  if (!n_edges) return fail(c, UVAIA_GPU_EINVAL, "NULL count of edges");
  *n_edges = 0;
  if (n_rounds) *n_rounds = 0;
  if (int rc = uvaia_gpu_db_near_begin(c, trim, metric, min_compared)) return rc;
  const size_t n = c->db_n;
  if (n < 2) return 0;
  if (!edges) return fail(c, UVAIA_GPU_EINVAL, "NULL edges");
  constexpr int MAX_ROUNDS = 64;                                 // (a round at least halves the components that still have an outgoing edge)
  std::vector<uint64_t> best(n);
  std::vector<uint32_t> parent(n), comp(n);
  struct Choice { uint32_t dist, lo, hi; };
  std::vector<Choice> choice(n);                                 // by component label (its smallest member); dist = NO: none
  std::iota(parent.begin(), parent.end(), 0u);
  auto find = [&parent](uint32_t x) { while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; } return x; };
  size_t found = 0;
  int rounds = 0;
  while (found < n - 1) {
    if (rounds == MAX_ROUNDS) return fail(c, UVAIA_GPU_ESTATE, "the spanning forest is not complete after %d rounds", MAX_ROUNDS);
    for (size_t x = 0; x < n; x++) comp[x] = find((uint32_t)x);  // unions go to the smaller root: the label is the smallest member
    if (rounds) if (int rc = uvaia_gpu_db_near_components(c, comp.data())) return rc;
    if (int rc = uvaia_gpu_db_near(c, 0, n, 0, n, nullptr)) return rc;
    if (int rc = uvaia_gpu_db_near_fetch(c, best.data())) return rc;
    rounds++;
    if (n_rounds) *n_rounds = rounds;
    for (size_t x = 0; x < n; x++) choice[x].dist = 0xFFFFFFFFu;
    for (size_t x = 0; x < n; x++) {
      if (best[x] == UVAIA_GPU_NEAR_NONE) continue;
      const uint32_t d = (uint32_t)(best[x] >> 32), y = (uint32_t)best[x];
      if (y >= n || y == x || comp[y] == comp[x]) return fail(c, UVAIA_GPU_ESTATE, "the key of reference %zu names reference %u of its own component", x, y);
      const Choice e = {d, std::min((uint32_t)x, y), std::max((uint32_t)x, y)};
      Choice &m = choice[comp[x]];
      if (std::tie(e.dist, e.lo, e.hi) < std::tie(m.dist, m.lo, m.hi)) m = e;
    }
    const size_t before = found;
    for (size_t r = 0; r < n; r++) {
      if (comp[r] != r || choice[r].dist == 0xFFFFFFFFu) continue;
      const uint32_t a = find(choice[r].lo), b = find(choice[r].hi);
      if (a == b) continue;                                      // the edge the component at its other end chose too
      parent[std::max(a, b)] = std::min(a, b);
      edges[found].a = choice[r].lo; edges[found].b = choice[r].hi; edges[found].dist = (int32_t)choice[r].dist;
      found++;
    }
    if (found == before) break;                                  // what is left has no edge between its components: a forest
  }
  std::sort(edges, edges + found, [](const uvaia_gpu_edge &p, const uvaia_gpu_edge &q) { return std::tie(p.dist, p.a, p.b) < std::tie(q.dist, q.a, q.b); });
  *n_edges = found;
  return 0;
}

void uvaia_gpu_near_ms(uvaia_gpu_ctx *c, double *ms, int reset)
{
  if (!c) return;
  if (ms) *ms = c->pairs.near_ms;
  if (reset) c->pairs.near_ms = 0.;
}

void uvaia_gpu_near_tiles(uvaia_gpu_ctx *c, unsigned long long out[2], int reset)
{
  if (!c) return;
  if (out) { out[0] = c->pairs.near_tiles[0]; out[1] = c->pairs.near_tiles[1]; }
  if (reset) c->pairs.near_tiles[0] = c->pairs.near_tiles[1] = 0;
}

}  // extern "C"
