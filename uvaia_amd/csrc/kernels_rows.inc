// kernels_rows.inc -- part of uvaia_gpu.hip (included there, not a translation unit of its own): a block of text rows that is already in device memory (the
// rows the aligner leaves behind, a tensor of the caller) on its way into the packed database: census, exception runs, ordered gather.
//
// A block is n rows of nchar bytes, `pitch` bytes apart; nothing is assumed about the pitch or about the alignment of the first row.  All three
// kernels take one thread block per row and walk it in pieces of 16 sites per thread, 4 KiB per round of the block: a row that starts on a
// 16-byte boundary is read with one dwordx4 load per piece (a wave reads 1 KiB contiguous), any other through five aligned dwords and
// v_alignbyte.  No dword is touched that holds no byte of the row.

constexpr int ROWS_TPB = 256;
constexpr uint32_t ROWS_RUN_CUT = 0xFFFFFFu;      // longest exception run of a packed database file (24 bits of a record, host/uvdb.c:83)

// per byte value: 1 = valid site (the rule of quick_count_sequence_non_N, host/seq_query.c:105-115: everything but N X O in either case and - ? .),
// 2 = exception character of the packed database (host/uvdb.c:81: - ? X O . as they are), 4 = refused by the engine (c_code, as pack_refs_kernel)
static __device__ __forceinline__ void rows_class_table(uint8_t *cls)
{
  const unsigned c = threadIdx.x, up = c & 0xDFu;
  const bool invalid = up == 'N' || up == 'X' || up == 'O' || c == '-' || c == '?' || c == '.';
  const bool exc = c == '-' || c == '?' || c == 'X' || c == 'O' || c == '.';
  cls[c] = (uint8_t)((invalid ? 0 : 1) | (exc ? 2 : 0) | (c_code[c] == 0xFFu ? 4 : 0));
  __syncthreads();
}

// sites site0 .. site0 + 15 of a row (site0 < nchar, a multiple of 16); bytes at and beyond nchar read 'N' (rows_block.h has the load)
static __device__ __forceinline__ uint4 rows_load16(const uint8_t *row, int nchar, int site0) { return rows_load16_fill<0x4E4E4E4Eu>(row, nchar, site0); }

// block-wide exclusive scans in thread order (all ROWS_TPB threads call them); wsh: four ints of LDS
static __device__ __forceinline__ uint32_t rows_scan_sum(uint32_t v, uint32_t *wsh, uint32_t &total)
{
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(incl, d, 64); if (lane >= d) incl += t; }
  if (lane == 63) wsh[wv] = incl;
  __syncthreads();
  uint32_t off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < ROWS_TPB / 64; w++) { const uint32_t x = wsh[w]; if (w < wv) off += x; tot += x; }
  __syncthreads();
  total = tot;
  return off + incl - v;
}

static __device__ __forceinline__ int rows_scan_max(int v, int *wsh, int &total)
{ // identity -1
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(incl, d, 64); if (lane >= d) incl = max(incl, t); }
  int excl = __shfl_up(incl, 1, 64);
  if (lane == 0) excl = -1;
  if (lane == 63) wsh[wv] = incl;
  __syncthreads();
  int off = -1, tot = -1;
#pragma unroll
  for (int w = 0; w < ROWS_TPB / 64; w++) { const int x = wsh[w]; if (w < wv) off = max(off, x); tot = max(tot, x); }
  __syncthreads();
  total = tot;
  return max(off, excl);
}

// One piece of a row: sites 16 k .. 16 k + 15 (have = the piece exists; the others only take part in the scans).
//   starts bit j: an exception record starts at site 16 k + j       ends bit j: one ends behind that site
//   valid: valid sites of the piece                                  bad: the piece holds a byte the engine refuses
// The rule is the loop of uvdb_add_reference (host/uvdb.c:79-94): a run is a maximal stretch of one exception character, cut every `cut`
// sites.  A record thus starts where a site is in the set and differs from its predecessor -- and, inside a stretch, every `cut` sites from
// there.  The second half can only happen in rows longer than `cut` (LONG): there a block-wide running maximum carries the start of the
// stretch a piece begins in (`carry`: over the rounds of the block).
template <bool LONG>
static __device__ __forceinline__ void rows_piece(const uint8_t *row, int nchar, int k, bool have, const uint8_t *cls, uint32_t cut, int &carry, int *wsh,
                                                  uint32_t &starts, uint32_t &ends, int &valid, int &bad)
{
  starts = ends = 0;
  uint8_t b[16];
  int prev = -1, next = -1, m = 0;
  const int site0 = k * 16;
  if (have) {
    const uint4 v = rows_load16(row, nchar, site0);
    memcpy(b, &v, 16);
    m = min(16, nchar - site0);
    if (site0 > 0) prev = row[site0 - 1];
    if (site0 + 16 < nchar) next = row[site0 + 16];
  }
  int a = -1;                                          // start of the stretch the walk is in
  if (LONG) {
    int ls = -1, p = prev;
    if (have) {
#pragma unroll
      for (int j = 0; j < 16; j++) if (j < m) { const int c = b[j]; if ((cls[c] & 2) && p != c) ls = site0 + j; p = c; }
    }
    int tot;
    a = max(rows_scan_max(ls, wsh, tot), carry);
    carry = max(carry, tot);
  }
  if (!have) return;
  int p = prev;
#pragma unroll
  for (int j = 0; j < 16; j++) {
    if (j < m) {
      const int c = b[j], f = cls[c], nx = (j + 1 < m) ? (int)b[(j + 1) & 15] : next, s = site0 + j;
      valid += f & 1; bad |= f & 4;
      if (f & 2) {
        const bool first = p != c;
        if (first) a = s;
        const bool st = LONG ? ((uint32_t)(s - a) % cut == 0) : first;
        const bool en = (nx != c) || (LONG && (uint32_t)(s + 1 - a) % cut == 0);
        starts |= (uint32_t)st << j; ends |= (uint32_t)en << j;
      }
      p = c;
    }
  }
}

// Row census: per row the valid-site count, the number of exception records its text gives, and the bad-byte flag (errflag |= 1, the d_err
// of pack_refs_kernel).  One block per row.
template <bool LONG>
__global__ __launch_bounds__(ROWS_TPB) void rows_census_kernel(const uint8_t *__restrict__ rows, size_t pitch, int nchar, uint32_t cut,
                                                               int *__restrict__ non_n, int *__restrict__ n_exc, int *__restrict__ errflag)
{
  __shared__ uint8_t cls[256];
  __shared__ int wsh[ROWS_TPB / 64];
  __shared__ int red[ROWS_TPB / 64][2];
  rows_class_table(cls);
  const uint8_t *row = rows + (size_t)blockIdx.x * pitch;
  const int n16 = (nchar + 15) >> 4;
  int valid = 0, records = 0, bad = 0, carry = -1;
  for (int k0 = 0; k0 < n16; k0 += ROWS_TPB) {
    const int k = k0 + (int)threadIdx.x;
    uint32_t st, en;
    rows_piece<LONG>(row, nchar, k, k < n16, cls, cut, carry, wsh, st, en, valid, bad);
    records += __popc(st);
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) { valid += __shfl_xor(valid, d, 64); records += __shfl_xor(records, d, 64); }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) { red[wv][0] = valid; red[wv][1] = records; }
  if (__ballot(bad != 0) && lane == 0) atomicOr(errflag, 1);
  __syncthreads();
  if (threadIdx.x == 0) {
    int v = 0, r = 0;
    for (int w = 0; w < ROWS_TPB / 64; w++) { v += red[w][0]; r += red[w][1]; }
    non_n[blockIdx.x] = v; n_exc[blockIdx.x] = r;
  }
}

// Exception fill, the second pass of the pair: block k writes the records (pos, len << 8 | char) of row row_index[k] (NULL: row k) to
// out[offsets[k] ..), by position.  Starts and ends of records are ranked by one block-wide prefix sum per round (the i-th end closes the i-th
// start); the thread that sees a start leaves its position, the one that sees the end leaves the end, and when the row is through the block
// turns the pairs into records.  A row whose records are not exactly offsets[k + 1] - offsets[k] (offsets that do not come from the census of
// these rows) writes nothing outside its range and raises errflag |= 2.
template <bool LONG>
__global__ __launch_bounds__(ROWS_TPB) void rows_fill_exceptions_kernel(const uint8_t *__restrict__ rows, size_t pitch, int nchar, uint32_t cut, const int *__restrict__ row_index,
                                                                        const unsigned long long *__restrict__ offsets, uint2 *out, int *__restrict__ errflag)
{
  __shared__ uint8_t cls[256];
  __shared__ int wsh[ROWS_TPB / 64];
  rows_class_table(cls);
  const int r = row_index ? row_index[blockIdx.x] : (int)blockIdx.x;
  const uint8_t *row = rows + (size_t)r * pitch;
  uint2 *o = out + offsets[blockIdx.x];
  const unsigned long long cap64 = offsets[blockIdx.x + 1] - offsets[blockIdx.x];
  const uint32_t cap = (uint32_t)min(cap64, (unsigned long long)0x7FFFFFFFu);
  const int n16 = (nchar + 15) >> 4;
  uint32_t base_s = 0, base_e = 0;
  int valid = 0, bad = 0, carry = -1;
  for (int k0 = 0; k0 < n16; k0 += ROWS_TPB) {
    const int k = k0 + (int)threadIdx.x;
    uint32_t st, en, total;
    rows_piece<LONG>(row, nchar, k, k < n16, cls, cut, carry, wsh, st, en, valid, bad);
    const uint32_t excl = rows_scan_sum((uint32_t)__popc(st) | ((uint32_t)__popc(en) << 16), reinterpret_cast<uint32_t *>(wsh), total);   // at most 4096 of each per round
    uint32_t ps = base_s + (excl & 0xFFFFu), pe = base_e + (excl >> 16);
    while (st) { const int j = __ffs(st) - 1; st &= st - 1; if (ps < cap) o[ps].x = (uint32_t)(k * 16 + j); ps++; }
    while (en) { const int j = __ffs(en) - 1; en &= en - 1; if (pe < cap) o[pe].y = (uint32_t)(k * 16 + j + 1); pe++; }
    base_s += total & 0xFFFFu; base_e += total >> 16;
  }
  __syncthreads();                                     // (the positions and ends left above are read by other threads of the block)
  if (base_s != cap || base_e != cap || cap64 != cap) { if (threadIdx.x == 0) atomicOr(errflag, 2); return; }
  for (uint32_t i = threadIdx.x; i < cap; i += ROWS_TPB) {
    const uint32_t pos = o[i].x, e = o[i].y;
    o[i].y = ((e - pos) << 8) | (uint32_t)row[pos];
  }
}

// Ordered gather: row row_index[first + k] (NULL: row first + k) of the block becomes row k of the engine's staging layout (dst_pitch a multiple
// of 16, dst 16-byte aligned: what pack_refs_kernel reads with two dwordx4 loads per word); the bytes between nchar and dst_pitch read 'N'.
__global__ __launch_bounds__(ROWS_TPB) void rows_gather_kernel(const uint8_t *__restrict__ rows, size_t pitch, int nchar, const int *__restrict__ row_index, int first,
                                                               uint8_t *__restrict__ dst, size_t dst_pitch)
{
  const int r = row_index ? row_index[first + (int)blockIdx.x] : first + (int)blockIdx.x;
  const uint8_t *row = rows + (size_t)r * pitch;
  uint4 *out = reinterpret_cast<uint4 *>(dst + (size_t)blockIdx.x * dst_pitch);
  const int n16 = (int)(dst_pitch >> 4);
  for (int t = threadIdx.x; t < n16; t += ROWS_TPB)
    out[t] = (t * 16 < nchar) ? rows_load16(row, nchar, t * 16) : make_uint4(0x4E4E4E4Eu, 0x4E4E4E4Eu, 0x4E4E4E4Eu, 0x4E4E4E4Eu);
}

// Side rows in one fixed form.  pack_refs_kernel lists a reference's partially ambiguous words in the order its four waves come across them
// (an atomic counter per lane): which order, and above AMB_CAP words which of them, depends on the timing of the waves, so two packings of the
// same text could differ in their side rows (never in what a search makes of them: any order and any AMB_CAP of the words are a valid row).
// For the resident database, whose rows end up in packed database files, this pass writes the row over from the packed planes themselves: the
// words in ascending order, the first AMB_CAP of them listed -- one of the rows pack_refs_kernel can leave, and always the same one.  A word
// is partially ambiguous when some site has two planes set (code & (code - 1), as there).  One wave per tile, lane = slot; four-plane stores.
__global__ __launch_bounds__(64) void side_rows_canonical_kernel(const uint4 *__restrict__ tiles, int W4, long long tile_base, long long slot0, int n_ref, int *__restrict__ amb_out)
{
  const long long tile = tile_base + blockIdx.x, slot = tile * 64 + threadIdx.x, i = slot - slot0;
  if (i < 0 || i >= n_ref) return;
  const uint4 *t = tiles + (size_t)tile * W4 * 4 * 64 + threadIdx.x;
  int *row = amb_out + (size_t)slot * AMB_ROW;
  int cnt = 0;
  for (int w4 = 0; w4 < W4; w4++) {
    const uint4 pA = t[(size_t)(w4 * 4 + 0) * 64], pC = t[(size_t)(w4 * 4 + 1) * 64], pG = t[(size_t)(w4 * 4 + 2) * 64], pT = t[(size_t)(w4 * 4 + 3) * 64];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t a = u4c(pA, j), c = u4c(pC, j), g = u4c(pG, j), tt = u4c(pT, j);
      if (((a & c) | (a & g) | (a & tt) | (c & g) | (c & tt) | (g & tt)) == 0) continue;
      if (cnt < AMB_CAP) { row[1 + cnt] = w4 * 4 + j; row[12 + 4 * cnt] = (int)a; row[13 + 4 * cnt] = (int)c; row[14 + 4 * cnt] = (int)g; row[15 + 4 * cnt] = (int)tt; }
      cnt++;
    }
  }
  row[0] = cnt;
  for (int k = cnt; k < AMB_CAP; k++) { row[1 + k] = 0; row[12 + 4 * k] = row[13 + 4 * k] = row[14 + 4 * k] = row[15 + 4 * k] = 0; }
}
