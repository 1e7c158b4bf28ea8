// kernels_fasta.inc -- part of uvaia_gpu.hip: a block of FASTA text in device memory split into records (pass 1) and into rows (pass 2).
//
// The rules are those of readfasta_next on a regular stream, restated with the lines they come from (paths under uvaia_amd/csrc/host):
//   * a line ends at '\n'; all trailing '\r' / '\n' bytes are not part of it (biomcmc_lite.c:274-277, biomcmc_getline_compress);
//   * a line with only white space -- 0x20 and 0x09-0x0D, isspace() of the C locale -- is skipped (seq_query.c:60, biomcmc_lite.c:131-136);
//   * a line that holds '>' anywhere is a header, its name the bytes after the FIRST '>' up to the end of the line (seq_query.c:61-68:
//     memchr over the whole line, strlen of what follows); the name may be empty and may hold spaces and further '>';
//   * the sequence of a record is the other lines up to the next header line, white space dropped, a-z upper-cased, every other byte kept
//     (seq_query.c:35 and 72-73, append_sequence_line);
//   * non_n counts the sites that are none of N n X x O o - ? . (seq_query.c:104-115, quick_count_sequence_non_N) over the record's own length.
// What the host reader does with irregular input is not restated: a NUL byte (it ends the C string of a line early), a line that is not blank
// before the first header (seq_query.c:72-73 appends it to a record without a name) and a record without one sequence byte (seq_query.c:69-70
// repeats the previous sequence under the new name or loses a name) are flagged, and the host entry refuses the text.
//
// Pass 1, three kernels and one more:
//   fasta_chunk_summary_kernel  per chunk of FASTA_CHUNK bytes: does it hold a '\n', is a header open at its end, where is its last '\n', how many
//                               of its '>' are the first of their line whatever came before the chunk, and is there one that is the first
//                               only if no header is open where the chunk begins
//   fasta_chunk_scan_kernel     one block: the exclusive scan of those summaries -- per chunk the state it begins in, the last '\n' before it and
//                               the number of header lines before it
//   fasta_headers_kernel        per chunk again, now with its carry: the position of every first '>' and of the start of its line, written at its
//                               rank.  An ordered compaction: counts, scan, write; no atomic decides an order.
//   fasta_records_kernel        one wave per record (and one for the text before the first header): name, body, cleaned length, non_n, flags.
// Pass 2, fasta_rows_kernel: one block per row.  The bytes a tile of FASTA_CHUNK keeps are compacted through LDS behind the remainder of the
// tile before and leave as 16-byte stores, so that a sequence on one line and one wrapped at 60 or 70 columns cost the same wide stores;
// upper-casing happens on the way into LDS.
//
// Every load is one aligned uint4 per lane, coalesced, whatever the alignment of the text: the first and last piece are masked to the range
// asked for.  Positions are clamped to the block length before they are used, and nothing is stored past the pitch of a row or the capacity
// of a table, whatever the tables say.

namespace {

constexpr int FASTA_TPB = 256;                  // threads per block of every kernel here
constexpr int FASTA_CHUNK = FASTA_TPB * 16;     // text bytes a block of pass 1 covers (aligned pieces of 16 bytes, one per lane)

enum : uint32_t { FASTA_F_NUL = 1u, FASTA_F_EMPTY = 2u, FASTA_F_TEXT = 4u };   // uvaia_gpu_fasta_record.flags (UVAIA_GPU_FASTA_* of the header)

struct FastaRec { uint32_t name_off, name_len, body_off, body_len, seq_len; int32_t non_n; uint32_t flags, bad_off; };   // = uvaia_gpu_fasta_record

// 16-bit masks over the bytes of one piece, bit j = byte j; only bytes whose position p0 + j lies in [lo, hi) count
struct FastaMasks { uint32_t valid, nl, gt, ws, nul, cr, inv; };

static __device__ __forceinline__ uint32_t fasta_byte(const uint4 &v, int j) { return (u4c(v, j >> 2) >> (8 * (j & 3))) & 0xFFu; }

static __device__ __forceinline__ FastaMasks fasta_classify(const uint4 &v, int p0, int lo, int hi)
{
  FastaMasks m = {0, 0, 0, 0, 0, 0, 0};
  const int a = min(max(lo - p0, 0), 16), b = min(max(hi - p0, 0), 16);
  m.valid = b > a ? ((1u << b) - 1u) & ~((1u << a) - 1u) : 0u;
#pragma unroll
  for (int j = 0; j < 16; j++) {
    const uint32_t c = fasta_byte(v, j), up = c & 0xDFu;
    m.nl |= (uint32_t)(c == '\n') << j;
    m.gt |= (uint32_t)(c == '>') << j;
    m.ws |= (uint32_t)((c == ' ') | ((c - 9u) < 5u)) << j;
    m.nul |= (uint32_t)(c == 0u) << j;
    m.cr |= (uint32_t)(c == '\r') << j;
    m.inv |= (uint32_t)((up == 'N') | (up == 'X') | (up == 'O') | (c == '-') | (c == '?') | (c == '.')) << j;
  }
  m.nl &= m.valid; m.gt &= m.valid; m.ws &= m.valid; m.nul &= m.valid; m.cr &= m.valid; m.inv &= m.valid;
  return m;
}

// the piece of lane `piece` (aligned, 16 bytes) of a text that begins `mis` bytes into its first piece; p0 = text position of its byte 0.
// Pieces that hold no byte of [0, n) are not loaded.
static __device__ __forceinline__ uint4 fasta_load(const uint4 *base, long long piece, int p0, int n)
{
  if (p0 >= n || p0 + 16 <= 0) return make_uint4(0, 0, 0, 0);
  return base[piece];
}

// Line state: bit 1 = a '\n' was seen, bit 0 = a header is open (a '>' since the last '\n').  then(a, b) = a followed by b.
static __device__ __forceinline__ int fasta_then(int a, int b) { return (b & 2) ? b : (a | b); }

// what a lane's 16 bytes do to the state, and its first-of-line '>' bits given that no header is open where it begins; `head` = the one
// bit among them that lies before the lane's first '\n' (it is no first if a header is open there)
static __device__ __forceinline__ void fasta_lane(uint32_t nl, uint32_t gt, int &state, uint32_t &firsts, uint32_t &head)
{
  uint32_t f = 0, open = 0;
#pragma unroll
  for (int j = 0; j < 16; j++) {
    const uint32_t isnl = (nl >> j) & 1u, isgt = (gt >> j) & 1u;
    f |= (isgt & ~open & 1u) << j;
    open = isnl ? 0u : (open | isgt);
  }
  const uint32_t headmask = nl ? ((nl & (0u - nl)) - 1u) : 0xFFFFu;
  const uint32_t hg = gt & headmask;
  head = hg & (0u - hg);
  firsts = f;
  state = (nl ? 2 : 0) | (int)open;
}

// exclusive scans over the block's lanes in lane order: the line state and the last '\n' position (max); `carry_*` is what the chunk begins with.
// sh: 2 * (FASTA_TPB / 64) ints of LDS.  Also gives the folds over the whole block.
static __device__ __forceinline__ void fasta_block_state_scan(int state, int lastnl, int carry_state, int carry_nl, int *sh, int &ex_state, int &ex_nl, int &all_state, int &all_nl)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int s = state, m = lastnl;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int ts = __shfl_up(s, d), tm = __shfl_up(m, d);
    if (lane >= d) { s = fasta_then(ts, s); m = max(m, tm); }
  }
  if (lane == 63) { sh[wave] = s; sh[FASTA_TPB / 64 + wave] = m; }
  int es = __shfl_up(s, 1), em = __shfl_up(m, 1);
  if (lane == 0) { es = 0; em = -1; }
  __syncthreads();
  int ps = carry_state, pm = carry_nl;
  all_state = carry_state; all_nl = carry_nl;
#pragma unroll
  for (int w = 0; w < FASTA_TPB / 64; w++) {
    if (w < wave) { ps = fasta_then(ps, sh[w]); pm = max(pm, sh[FASTA_TPB / 64 + w]); }
    all_state = fasta_then(all_state, sh[w]); all_nl = max(all_nl, sh[FASTA_TPB / 64 + w]);
  }
  ex_state = fasta_then(ps, es); ex_nl = max(pm, em);
  __syncthreads();
}

// exclusive sum of v over the block's lanes in lane order, and the block's total.  sh: FASTA_TPB / 64 ints of LDS.
static __device__ __forceinline__ int fasta_block_sum_scan(int v, int *sh, int &total)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int s = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(s, d); if (lane >= d) s += t; }
  if (lane == 63) sh[wave] = s;
  __syncthreads();
  int pre = 0; total = 0;
#pragma unroll
  for (int w = 0; w < FASTA_TPB / 64; w++) { if (w < wave) pre += sh[w]; total += sh[w]; }
  __syncthreads();
  return pre + s - v;
}

// summary[c] = (state of the chunk, first '>' that count whatever came before, 1 if one more counts when no header is open before, last '\n' or -1)
__global__ __launch_bounds__(FASTA_TPB) void fasta_chunk_summary_kernel(const uint4 *base, int mis, int n, int4 *summary)
{
  __shared__ int sh[2 * (FASTA_TPB / 64)];
  const long long piece = (long long)blockIdx.x * FASTA_TPB + threadIdx.x;
  const int p0 = (int)(piece * 16 - mis);
  const FastaMasks m = fasta_classify(fasta_load(base, piece, p0, n), p0, 0, n);
  int state; uint32_t firsts, head;
  fasta_lane(m.nl, m.gt, state, firsts, head);
  const int lastnl = m.nl ? p0 + 31 - __clz(m.nl) : -1;
  int ex_state, ex_nl, all_state, all_nl;
  fasta_block_state_scan(state, lastnl, 0, -1, sh, ex_state, ex_nl, all_state, all_nl);
  if (ex_state & 1) firsts &= ~head;                                   // a header of this chunk is open where the lane begins
  const int is_head = (head != 0u) && !(ex_state & 1) && !(ex_state & 2);   // ... or may be, from before the chunk
  int total, heads;
  fasta_block_sum_scan(__popc(firsts), sh, total);
  fasta_block_sum_scan(is_head, sh, heads);
  if (threadIdx.x == 0) summary[blockIdx.x] = make_int4(all_state, total - heads, heads, all_nl);
}

// in place: summary[c] = (state the chunk begins in, header lines before it, 0, last '\n' before it); *total = header lines in all
__global__ __launch_bounds__(FASTA_TPB) void fasta_chunk_scan_kernel(int4 *summary, int n_chunks, int *total)
{
  __shared__ int s_state[FASTA_TPB], s_cnt[2][FASTA_TPB], s_nl[FASTA_TPB], s_open[FASTA_TPB];
  const int per = (n_chunks + FASTA_TPB - 1) / FASTA_TPB, t = threadIdx.x;
  const int a = min(t * per, n_chunks), b = min(a + per, n_chunks);
  int st = 0, nl = -1, c0 = 0, c1 = 0, o0 = 0, o1 = 1;          // the range's fold; its header count begun with no header open, and with one
  for (int c = a; c < b; c++) {
    const int4 v = summary[c];
    c0 += v.y + (v.z && !o0); c1 += v.y + (v.z && !o1);
    o0 = fasta_then(o0, v.x) & 1; o1 = fasta_then(o1, v.x) & 1;
    st = fasta_then(st, v.x); nl = max(nl, v.w);
  }
  s_state[t] = st; s_cnt[0][t] = c0; s_cnt[1][t] = c1; s_nl[t] = nl;
  __syncthreads();
  if (t == 0) {
    int cs = 0, cn = -1, cc = 0;
    for (int i = 0; i < FASTA_TPB; i++) {
      const int mine = s_cnt[cs & 1][i], fs = s_state[i], fn = s_nl[i];
      s_open[i] = cs; s_cnt[0][i] = cc; s_nl[i] = cn;
      cc += mine; cs = fasta_then(cs, fs); cn = max(cn, fn);
    }
    *total = cc;
  }
  __syncthreads();
  int cs = s_open[t], cc = s_cnt[0][t], cn = s_nl[t];
  for (int c = a; c < b; c++) {
    const int4 v = summary[c];
    summary[c] = make_int4(cs, cc, 0, cn);
    cc += v.y + (v.z && !(cs & 1)); cs = fasta_then(cs, v.x); cn = max(cn, v.w);
  }
}

// hdr_gt[k] = position of the first '>' of the k-th header line, hdr_line[k] = where that line begins, for k < cap
__global__ __launch_bounds__(FASTA_TPB) void fasta_headers_kernel(const uint4 *base, int mis, int n, const int4 *carry, int cap, int *hdr_gt, int *hdr_line)
{
  __shared__ int sh[2 * (FASTA_TPB / 64)];
  const long long piece = (long long)blockIdx.x * FASTA_TPB + threadIdx.x;
  const int p0 = (int)(piece * 16 - mis);
  const FastaMasks m = fasta_classify(fasta_load(base, piece, p0, n), p0, 0, n);
  const int4 cy = carry[blockIdx.x];
  int state; uint32_t firsts, head;
  fasta_lane(m.nl, m.gt, state, firsts, head);
  const int lastnl = m.nl ? p0 + 31 - __clz(m.nl) : -1;
  int ex_state, ex_nl, all_state, all_nl;
  fasta_block_state_scan(state, lastnl, cy.x, cy.w, sh, ex_state, ex_nl, all_state, all_nl);
  if (ex_state & 1) firsts &= ~head;
  int total;
  long long k = (long long)cy.y + fasta_block_sum_scan(__popc(firsts), sh, total);
  while (firsts && k < cap) {
    const int j = __ffs(firsts) - 1;
    firsts &= firsts - 1u;
    const uint32_t below = m.nl & ((1u << j) - 1u);
    hdr_gt[k] = p0 + j;
    hdr_line[k] = 1 + (below ? p0 + 31 - __clz(below) : ex_nl);
    k++;
  }
}

static __device__ __forceinline__ int fasta_wave_min(int v) { for (int d = 32; d; d >>= 1) v = min(v, __shfl_xor(v, d)); return v; }
static __device__ __forceinline__ int fasta_wave_max(int v) { for (int d = 32; d; d >>= 1) v = max(v, __shfl_xor(v, d)); return v; }
static __device__ __forceinline__ int fasta_wave_sum(int v) { for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d); return v; }

// One wave per record k < n_rec: rec[k].  The wave after them takes the text before the first header line: rec[n_rec] with body_len = its
// length, name_off = its first byte that is no white space (FASTA_F_TEXT), bad_off = its first NUL (FASTA_F_NUL).
// n_known: entries of hdr_* that are filled; a record ends where the next known header line begins, the last one at n.
__global__ __launch_bounds__(FASTA_TPB) void fasta_records_kernel(const uint4 *base, int mis, int n, int n_rec, int n_known, const int *hdr_gt, const int *hdr_line, FastaRec *rec)
{
  const int lane = threadIdx.x & 63;
  const long long w = (long long)blockIdx.x * (FASTA_TPB / 64) + (threadIdx.x >> 6);
  if (w > n_rec) return;
  const int big = 0x7FFFFFFF;
  if (w == n_rec) {                                       // the text before the first header line
    const int end = n_known > 0 ? min(max(hdr_line[0], 0), n) : n;
    int first_text = big, first_nul = big;
    for (long long pc = mis / 16; pc * 16 - mis < end; pc += 64) {
      const int p0 = (int)((pc + lane) * 16 - mis);
      const FastaMasks m = fasta_classify(fasta_load(base, pc + lane, p0, end), p0, 0, end);
      const uint32_t text = m.valid & ~m.ws;
      if (text) first_text = min(first_text, p0 + __ffs(text) - 1);
      if (m.nul) first_nul = min(first_nul, p0 + __ffs(m.nul) - 1);
    }
    first_text = fasta_wave_min(first_text); first_nul = fasta_wave_min(first_nul);
    if (lane == 0) {
      FastaRec r = {0, 0, 0, (uint32_t)end, 0, 0, 0, 0};
      if (first_text != big) { r.flags |= FASTA_F_TEXT; r.name_off = (uint32_t)first_text; }
      if (first_nul != big) { r.flags |= FASTA_F_NUL; r.bad_off = (uint32_t)first_nul; }
      rec[n_rec] = r;
    }
    return;
  }
  const int k = (int)w;
  const int start = min(max(hdr_line[k], 0), n);
  const int end = k + 1 < n_known ? min(max(hdr_line[k + 1], start), n) : n;
  const int g = min(max(hdr_gt[k], start), end);
  // the header line: its '\n' (or the end of the record), the last byte of the name that is no '\r', a NUL
  int nlpos = big, first_nul = big;
  const long long pg = ((long long)g + mis) / 16;
  for (long long pc = pg; pc * 16 - mis < end && nlpos == big; pc += 64) {
    const int p0 = (int)((pc + lane) * 16 - mis);
    const FastaMasks m = fasta_classify(fasta_load(base, pc + lane, p0, end), p0, g, end);
    nlpos = fasta_wave_min(m.nl ? p0 + __ffs(m.nl) - 1 : big);
  }
  if (nlpos == big) nlpos = end;
  int last_name = -1;
  for (long long pc = ((long long)start + mis) / 16; pc * 16 - mis < nlpos; pc += 64) {
    const int p0 = (int)((pc + lane) * 16 - mis);
    const uint4 v = fasta_load(base, pc + lane, p0, nlpos);
    const FastaMasks m = fasta_classify(v, p0, start, nlpos);
    if (m.nul) first_nul = min(first_nul, p0 + __ffs(m.nul) - 1);
    const FastaMasks mn = fasta_classify(v, p0, g + 1, nlpos);
    const uint32_t keep = mn.valid & ~mn.cr;
    if (keep) last_name = max(last_name, p0 + 31 - __clz(keep));
  }
  last_name = fasta_wave_max(last_name);
  // the body
  const int body = min(nlpos + 1, end);
  int sites = 0, invalid = 0;
  for (long long pc = ((long long)body + mis) / 16; pc * 16 - mis < end; pc += 64) {
    const int p0 = (int)((pc + lane) * 16 - mis);
    const FastaMasks m = fasta_classify(fasta_load(base, pc + lane, p0, end), p0, body, end);
    sites += __popc(m.valid & ~m.ws); invalid += __popc(m.inv);
    if (m.nul) first_nul = min(first_nul, p0 + __ffs(m.nul) - 1);
  }
  sites = fasta_wave_sum(sites); invalid = fasta_wave_sum(invalid); first_nul = fasta_wave_min(first_nul);
  if (lane == 0) {
    FastaRec r;
    r.name_off = (uint32_t)min(g + 1, end); r.name_len = last_name > g ? (uint32_t)(last_name - g) : 0u;
    r.body_off = (uint32_t)body; r.body_len = (uint32_t)(end - body);
    r.seq_len = (uint32_t)sites; r.non_n = sites - invalid;
    r.flags = (first_nul != big ? FASTA_F_NUL : 0u) | (sites == 0 ? FASTA_F_EMPTY : 0u);
    r.bad_off = first_nul != big ? (uint32_t)first_nul : 0u;
    rec[k] = r;
  }
}

// Row r = the cleaned text of body[r] = (offset, length) in the block, at rows + r * pitch (pitch a multiple of 16, rows 16-byte aligned);
// at most nchar bytes of it, the rest of the last 16-byte piece zero.
__global__ __launch_bounds__(FASTA_TPB) void fasta_rows_kernel(const uint4 *base, int mis, int n, const int2 *body, int nchar, uint8_t *rows, size_t pitch)
{
  __shared__ __attribute__((aligned(16))) unsigned char stage[FASTA_CHUNK + 32];
  __shared__ int sh[FASTA_TPB / 64];
  const int2 bd = body[blockIdx.x];
  const int lo = min(max(bd.x, 0), n), hi = (int)min((long long)lo + max(bd.y, 0), (long long)n);
  uint8_t *out = rows + (size_t)blockIdx.x * pitch;
  int carry = 0, flushed = 0;                               // bytes waiting at the front of stage; bytes of the row already stored
  for (long long pc = ((long long)lo + mis) / 16; pc * 16 - mis < hi; pc += FASTA_TPB) {
    const int p0 = (int)((pc + threadIdx.x) * 16 - mis);
    const uint4 v = fasta_load(base, pc + threadIdx.x, p0, hi);
    const FastaMasks m = fasta_classify(v, p0, lo, hi);
    const uint32_t keep = m.valid & ~m.ws;
    int total;
    int at = carry + fasta_block_sum_scan(__popc(keep), sh, total);
    const int room = nchar - flushed;                       // stage positions from `room` on would lie past the row
    if (keep == 0xFFFFu && !(at & 3) && at + 16 <= room) {  // nothing dropped and a word-aligned place: four words
      uint32_t *d = reinterpret_cast<uint32_t *>(stage + at);
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const uint32_t x = u4c(v, q);
        // upper-case the four bytes at once: bytes in 'a'..'z' lose 0x20 (no carries between bytes: the high bits are masked off first)
        const uint32_t l = x & 0x7F7F7F7Fu, ge = l + 0x1F1F1F1Fu, gt = l + 0x05050505u;     // bit 7: >= 'a'; > 'z'
        const uint32_t is = ge & ~gt & ~x & 0x80808080u;
        d[q] = x ^ (is >> 2);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 16; j++) {
        if ((keep >> j) & 1u) {
          uint32_t c = fasta_byte(v, j);
          c -= ((c - 'a') < 26u) ? 32u : 0u;
          if (at < room) stage[at] = (unsigned char)c;
          at++;
        }
      }
    }
    __syncthreads();
    const int avail = max(min(carry + total, room), 0), nfull = avail / 16, rest = avail - nfull * 16;
    for (int i = threadIdx.x; i < nfull; i += FASTA_TPB)
      if ((size_t)flushed + (size_t)i * 16 + 16 <= pitch) *reinterpret_cast<uint4 *>(out + flushed + (size_t)i * 16) = *reinterpret_cast<const uint4 *>(stage + (size_t)i * 16);
    unsigned char keepb = 0;
    if ((int)threadIdx.x < rest) keepb = stage[nfull * 16 + threadIdx.x];
    __syncthreads();
    if ((int)threadIdx.x < rest) stage[threadIdx.x] = keepb;
    flushed += nfull * 16; carry = rest;
    __syncthreads();
  }
  if (carry > 0) {
    if ((int)threadIdx.x >= carry && threadIdx.x < 16) stage[threadIdx.x] = 0;
    __syncthreads();
    if (threadIdx.x == 0 && (size_t)flushed + 16 <= pitch) *reinterpret_cast<uint4 *>(out + flushed) = *reinterpret_cast<const uint4 *>(stage);
  }
}

// acgt[k] = the body bytes of record k that are one of A C G T a c g t (the first counter of biomcmc_count_sequence_acgt,
// biomcmc_lite.c:378-392); one wave per record, over the body the record table names.
__global__ __launch_bounds__(FASTA_TPB) void fasta_acgt_kernel(const uint4 *base, int mis, int n, int n_rec, const FastaRec *rec, int *acgt)
{
  const int lane = threadIdx.x & 63;
  const long long w = (long long)blockIdx.x * (FASTA_TPB / 64) + (threadIdx.x >> 6);
  if (w >= n_rec) return;
  const FastaRec r = rec[w];
  const int lo = (int)min((unsigned long long)r.body_off, (unsigned long long)n), hi = (int)min((unsigned long long)lo + r.body_len, (unsigned long long)n);
  int count = 0;
  for (long long pc = ((long long)lo + mis) / 16; pc * 16 - mis < hi; pc += 64) {
    const int p0 = (int)((pc + lane) * 16 - mis);
    const uint4 v = fasta_load(base, pc + lane, p0, hi);
    const int a = min(max(lo - p0, 0), 16), b = min(max(hi - p0, 0), 16);
    const uint32_t valid = b > a ? ((1u << b) - 1u) & ~((1u << a) - 1u) : 0u;
    uint32_t is = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const uint32_t up = fasta_byte(v, j) & 0xDFu;
      is |= (uint32_t)((up == 'A') | (up == 'C') | (up == 'G') | (up == 'T')) << j;
    }
    count += __popc(is & valid);
  }
  count = fasta_wave_sum(count);
  if (lane == 0) acgt[w] = count;
}

// Sequence k = the cleaned text of body[k] = (offset, length) in the block, at out[dst[k] .. dst[k + 1]): any byte offset, any length, the
// sequences back to back.  As fasta_rows_kernel, one block per sequence and the kept bytes compacted through LDS; the stage is seeded with
// dst[k] & 15 phantom bytes, so that stage position s is the byte out[(dst[k] & ~15) + s] and whole pieces leave as aligned 16-byte stores.
// The piece the sequence begins in and the one it ends in may belong to its neighbours as well, whose blocks run at the same time: of
// those only the bytes in [dst[k], dst[k + 1]) are stored, one by one.  total = bytes of out that sequences may take: nothing is stored
// at or past it.
__global__ __launch_bounds__(FASTA_TPB) void fasta_sequences_kernel(const uint4 *base, int mis, int n, const int2 *body, const long long *dst, long long total, uint8_t *out)
{
  __shared__ __attribute__((aligned(16))) unsigned char stage[FASTA_CHUNK + 32];
  __shared__ int sh[FASTA_TPB / 64];
  const int2 bd = body[blockIdx.x];
  const int lo = min(max(bd.x, 0), n), hi = (int)min((long long)lo + max(bd.y, 0), (long long)n);
  const long long d0 = min(max(dst[blockIdx.x], 0ll), total), d1 = min(max(dst[blockIdx.x + 1], d0), total);
  const int phantom = (int)(d0 & 15);
  const int last = phantom + (int)min(d1 - d0, (long long)0x40000000);     // stage positions [phantom, last) are the sequence
  uint8_t *line = out + (d0 - phantom);                                    // 16-byte aligned: out is
  int carry = phantom, flushed = 0;                                        // bytes waiting at the front of stage; stage positions already stored
  for (long long pc = ((long long)lo + mis) / 16; pc * 16 - mis < hi; pc += FASTA_TPB) {
    const int p0 = (int)((pc + threadIdx.x) * 16 - mis);
    const uint4 v = fasta_load(base, pc + threadIdx.x, p0, hi);
    const FastaMasks m = fasta_classify(v, p0, lo, hi);
    const uint32_t keep = m.valid & ~m.ws;
    int total_kept;
    int at = carry + fasta_block_sum_scan(__popc(keep), sh, total_kept);
    const int room = last - flushed;                        // stage positions from `room` on would lie past the sequence
    if (keep == 0xFFFFu && !(at & 3) && at + 16 <= room) {  // nothing dropped and a word-aligned place: four words (upper-cased as in fasta_rows_kernel)
      uint32_t *d = reinterpret_cast<uint32_t *>(stage + at);
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const uint32_t x = u4c(v, q);
        const uint32_t l = x & 0x7F7F7F7Fu, ge = l + 0x1F1F1F1Fu, gt = l + 0x05050505u;
        const uint32_t is = ge & ~gt & ~x & 0x80808080u;
        d[q] = x ^ (is >> 2);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 16; j++) {
        if ((keep >> j) & 1u) {
          uint32_t c = fasta_byte(v, j);
          c -= ((c - 'a') < 26u) ? 32u : 0u;
          if (at < room) stage[at] = (unsigned char)c;
          at++;
        }
      }
    }
    __syncthreads();
    const int avail = max(min(carry + total_kept, room), 0), nfull = avail / 16, rest = avail - nfull * 16;
    for (int i = threadIdx.x; i < nfull; i += FASTA_TPB) {
      const int s = flushed + i * 16;                       // (s + 16 <= last: the piece ends inside the sequence)
      if (s >= phantom) *reinterpret_cast<uint4 *>(line + s) = *reinterpret_cast<const uint4 *>(stage + (size_t)i * 16);
      else for (int j = phantom; j < 16; j++) line[j] = stage[j];     // the piece the sequence begins in (s = 0)
    }
    unsigned char keepb = 0;
    if ((int)threadIdx.x < rest) keepb = stage[nfull * 16 + threadIdx.x];
    __syncthreads();
    if ((int)threadIdx.x < rest) stage[threadIdx.x] = keepb;
    flushed += nfull * 16; carry = rest;
    __syncthreads();
  }
  // the piece the sequence ends in (and begins in, if it is that short)
  const int s = flushed + (int)threadIdx.x;
  if ((int)threadIdx.x < carry && s >= phantom && s < last) line[s] = stage[threadIdx.x];
}

}  // namespace
