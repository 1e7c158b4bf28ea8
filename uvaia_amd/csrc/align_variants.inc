// align_variants.inc -- what a row on the reference's columns differs from the reference by (uvaia_align_set_variants, uvaia_align_variants_of
// of include/uvaia_align.h): substitutions, deletion runs and the per-row counts.  Included by uvaia_align.hip inside its unnamed namespace;
// nothing here is part of the aligner's kernels.
//
// Bytes are classified as they are: A C G T are bases, '-' is a gap, 'N' is unknown, anything else is "other".  A substitution is a base that
// differs from the reference's byte; a deletion is a maximal run of gaps.
//
// Three launches over n rows, `pitch` bytes apart (any pitch >= ref_len, any alignment: rows_load16_fill):
//   variants_count_kernel    one wave per row, 64 lanes x 16 sites a round: one 32-byte uvaia_align_row_qc per row;
//   variants_offsets_kernel  one block: the exclusive scan of substitutions + deletion_runs over the rows (off[n] = records in all);
//   variants_emit_kernel     the walk of the count pass again: every lane writes its records at off[row] + records of the earlier rounds +
//                            records of the lower lanes.  One 16-byte store per record, every slot has one writer, no atomics.
// A deletion is counted and written where it CLOSES: at the first site behind the run that is no gap (site ref_len for a run that reaches
// the row's end), so a lane needs no byte of the lanes above it.  No substitution lies inside a run, so the order by closing site is the
// order by first site against every other record, and a deletion that closes at a substituted site goes first.  Its first site is the site
// behind the last non-gap below the closing site: in the lane's own 16 sites, or a running maximum over the lower lanes and earlier rounds.

static_assert(sizeof(uvaia_align_variant) == sizeof(int4), "a record is one 16-byte store");
static_assert(sizeof(uvaia_align_row_qc) == 2 * sizeof(int4), "a row's counts are two 16-byte stores");

struct VarLane {          // 16 sites of one lane: bit j = site site0 + j; nothing is set at and beyond ref_len
  uint4 q, r;             // the row's bytes and the reference's
  uint32_t valid, gap, sub, mat, unk, oth;
  uint32_t close;         // deletions that close at a site of this lane (a site up to ref_len itself)
};

__device__ __forceinline__ uint32_t byte_of(const uint4 &v, int j)
{
  const uint64_t lo = (uint64_t)v.x | ((uint64_t)v.y << 32), hi = (uint64_t)v.z | ((uint64_t)v.w << 32);
  return (uint32_t)(((j < 8 ? lo : hi) >> (8 * (j & 7))) & 0xFFu);
}

// gap_before: whether the site before this round's first is a gap (wave-uniform); it leaves as the same for the next round
__device__ __forceinline__ VarLane variant_lane(const uint8_t *row, const uint8_t *ref, int ref_len, int site0, int lane, uint32_t &gap_before)
{
  VarLane m;
  m.q = m.r = make_uint4(0, 0, 0, 0);
  m.valid = m.gap = m.sub = m.mat = m.unk = m.oth = 0;
  if (site0 < ref_len) {
    m.q = rows_load16_fill<0u>(row, ref_len, site0);
    m.r = rows_load16_fill<0u>(ref, ref_len, site0);
    const uint32_t qw[4] = {m.q.x, m.q.y, m.q.z, m.q.w}, rw[4] = {m.r.x, m.r.y, m.r.z, m.r.w};
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const uint32_t c = (qw[j >> 2] >> (8 * (j & 3))) & 0xFFu, d = (rw[j >> 2] >> (8 * (j & 3))) & 0xFFu;
      const uint32_t base = c == 'A' || c == 'C' || c == 'G' || c == 'T', gap = c == '-', unk = c == 'N';
      m.gap |= gap << j;
      m.unk |= unk << j;
      m.oth |= (uint32_t)(!base && !gap && !unk) << j;
      m.sub |= (uint32_t)(base && c != d) << j;
      m.mat |= (uint32_t)(base && c == d) << j;
    }
    const int rem = ref_len - site0;
    m.valid = rem >= 16 ? 0xFFFFu : ((1u << rem) - 1u);
    m.gap &= m.valid; m.unk &= m.valid; m.oth &= m.valid; m.sub &= m.valid; m.mat &= m.valid;
  }
  uint32_t prev = (uint32_t)__shfl_up((int)(m.gap >> 15), 1);
  if (lane == 0) prev = gap_before;
  gap_before = (uint32_t)__builtin_amdgcn_readlane((int)m.gap, 63) >> 15;
  const int nb = ref_len - site0 + 1;                                   // sites of this lane up to ref_len itself
  const uint32_t may_close = nb >= 16 ? 0xFFFFu : (nb > 0 ? ((1u << nb) - 1u) : 0u);
  m.close = ~m.gap & ((m.gap << 1) | prev) & may_close;
  return m;
}

__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ __launch_bounds__(256) void variants_count_kernel(const uint8_t *__restrict__ rows, size_t pitch, int n, const uint8_t *__restrict__ ref, int ref_len, int4 *__restrict__ qc)
{
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n) return;
  const uint8_t *t = rows + (size_t)row * pitch;
  int mat = 0, sub = 0, runs = 0, del = 0, unk = 0, oth = 0, first = ref_len, last = -1;
  uint32_t gap_before = 0;
  for (int base = 0; base <= ref_len; base += 1024) {                  // (site ref_len is where a run that reaches the row's end closes)
    const int site0 = base + lane * 16;
    const VarLane m = variant_lane(t, ref, ref_len, site0, lane, gap_before);
    mat += __popc(m.mat); sub += __popc(m.sub); runs += __popc(m.close); del += __popc(m.gap); unk += __popc(m.unk); oth += __popc(m.oth);
    const uint32_t there = m.valid & ~m.gap;
    if (there) { first = min(first, site0 + __builtin_ctz(there)); last = max(last, site0 + 31 - __clz((int)there)); }
  }
  mat = wave_sum(mat); sub = wave_sum(sub); runs = wave_sum(runs); del = wave_sum(del); unk = wave_sum(unk); oth = wave_sum(oth);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { first = min(first, __shfl_xor(first, o)); last = max(last, __shfl_xor(last, o)); }
  if (lane == 0) {
    qc[2 * (size_t)row] = make_int4(mat, sub, runs, del);
    qc[2 * (size_t)row + 1] = make_int4(unk, oth, first, last);
  }
}

// off[i] = records of the rows before row i, off[n] = records in all.  One block: thread t takes rows [t * per, (t + 1) * per).
__global__ __launch_bounds__(1024) void variants_offsets_kernel(const int4 *__restrict__ qc, int n, long long *__restrict__ off)
{
  __shared__ long long part[16];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long long per = ((long long)n + 1023) / 1024, a = min((long long)t * per, (long long)n), b = min(a + per, (long long)n);
  long long s = 0;
  for (long long i = a; i < b; i++) { const int4 c = qc[2 * i]; s += (long long)c.y + c.z; }
  long long v = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const long long u = __shfl_up(v, o); if (lane >= o) v += u; }
  if (lane == 63) part[wave] = v;
  __syncthreads();
  long long run = v - s;
  for (int w = 0; w < wave; w++) run += part[w];
  for (long long i = a; i < b; i++) { off[i] = run; const int4 c = qc[2 * i]; run += (long long)c.y + c.z; }
  if (t == 1023) off[n] = run;
}

__global__ __launch_bounds__(256) void variants_emit_kernel(const uint8_t *__restrict__ rows, size_t pitch, int n, const uint8_t *__restrict__ ref, int ref_len,
                                                            const long long *__restrict__ off, int4 *__restrict__ rec)
{
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n) return;
  const uint8_t *t = rows + (size_t)row * pitch;
  long long at = off[row];
  uint32_t gap_before = 0;
  int open = 0;                                                        // first site of the run that is open where this round starts, if one is
  for (int base = 0; base <= ref_len; base += 1024) {
    const int site0 = base + lane * 16;
    const VarLane m = variant_lane(t, ref, ref_len, site0, lane, gap_before);
    // the site behind the last non-gap so far: ascending with the lane, so a running maximum is the latest one
    const uint32_t nongap = ~m.gap & 0xFFFFu;
    int v = nongap ? site0 + 32 - __clz((int)nongap) : -1;
    if (lane == 0) v = max(v, open);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(v, o); if (lane >= o) v = max(v, u); }
    int below_start = __shfl_up(v, 1);
    if (lane == 0) below_start = open;
    open = __builtin_amdgcn_readlane(v, 63);
    const int cnt = __popc(m.close) + __popc(m.sub);
    int incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(incl, o); if (lane >= o) incl += u; }
    long long p = at + (incl - cnt);
    at += __builtin_amdgcn_readlane(incl, 63);
    uint32_t ev = m.close | m.sub;
    while (ev) {
      const int i = __builtin_ctz(ev);
      ev &= ev - 1;
      if ((m.close >> i) & 1u) {
        const uint32_t below = nongap & ((1u << i) - 1u);
        const int start = below ? site0 + 32 - __clz((int)below) : below_start;
        rec[p++] = make_int4(row, start, site0 + i - start, (int)'D');
      }
      if ((m.sub >> i) & 1u) rec[p++] = make_int4(row, site0 + i, 1, (int)((uint32_t)'S' | (byte_of(m.r, i) << 8) | (byte_of(m.q, i) << 16)));
    }
  }
}
