// kernels_pack.inc -- part of uvaia_gpu.hip (included there, not a translation unit of its own): packing raw characters into tile-interleaved bit-planes, import of packed tiles.

// ------------------------------------------------------------------------------------------------------------
// device: packing raw characters into tile-interleaved bit-planes
// ------------------------------------------------------------------------------------------------------------
__constant__ uint8_t c_code[256];

// One block per tile of 64 database slots; wave v handles word groups w4 = v, v+4, ...  Slots outside
// [slot0, slot0+n_ref) are left untouched (the database is zero-initialised), so appends need not be tile-aligned.
// non_n_out (nullable): valid-site count over the FULL length (src/fastaseq.c:642-648).
// amb_out (nullable): per slot a side row of AMB_ROW ints = number of alignment words holding a partially ambiguous (valid,
// non-ACGT) site, up to AMB_CAP of their indices and the four plane words of each; a count above AMB_CAP means "list
// incomplete, rescan densely".
template <int P>
__global__ __launch_bounds__(256) void pack_refs_kernel(const uint8_t *__restrict__ chars, size_t pitch, int nchar,
                                                         long long slot0, int n_ref, int W4, uint4 *__restrict__ tiles,
                                                         long long tile_base, int *__restrict__ non_n_out, int *__restrict__ amb_out,
                                                         int *__restrict__ tot_out, int *__restrict__ errflag)
{
  __shared__ uint8_t lut[256];
  __shared__ int partial[4][64];
  __shared__ int partial_acgt[4][64];
  __shared__ int amb_n[64];
  __shared__ int amb_w[64][AMB_CAP];
  __shared__ uint32_t amb_p[64][AMB_CAP][4];
  lut[threadIdx.x] = c_code[threadIdx.x];
  if (threadIdx.x < 64) amb_n[threadIdx.x] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long tile = tile_base + blockIdx.x;
  const long long slot = tile * 64 + lane;
  const long long i = slot - slot0;                  // row in chars
  const bool active = (i >= 0 && i < n_ref);
  const uint8_t *row = chars + (active ? (size_t)i * pitch : 0);
  const bool vec = ((pitch & 15) == 0) && ((((uintptr_t)chars) & 15) == 0);
  int valid = 0, n_acgt = 0, bad = 0;
  for (int w4 = wv; w4 < W4; w4 += 4) {
    uint32_t pl[4][4];                               // [plane][j]
#pragma unroll
    for (int p = 0; p < 4; p++) { pl[p][0] = pl[p][1] = pl[p][2] = pl[p][3] = 0; }
    if (active) {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int site0 = (w4 * 4 + j) * 32;
        if (site0 >= nchar) break;
        uint8_t b[32];
        if (vec && site0 + 32 <= (int)pitch) {
          const uint4 *v = reinterpret_cast<const uint4 *>(row + site0);
          uint4 x0 = v[0], x1 = v[1];
          memcpy(b, &x0, 16); memcpy(b + 16, &x1, 16);
        } else {
          for (int s = 0; s < 32; s++) b[s] = (site0 + s < nchar) ? row[site0 + s] : (uint8_t)'N';
        }
        uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0, partial_code = 0;
#pragma unroll
        for (int s = 0; s < 32; s++) {
          uint32_t code = (site0 + s < nchar) ? lut[b[s]] : 0u;
          if (code == 0xFFu) { bad = 1; code = 0; }
          valid += (code != 0);
          n_acgt += (code != 0) & ((code & (code - 1)) == 0);
          partial_code |= code & (code - 1);
          if (P == 4) {
            a0 |= (code & 1u) << s; a1 |= ((code >> 1) & 1u) << s; a2 |= ((code >> 2) & 1u) << s; a3 |= ((code >> 3) & 1u) << s;
          } else {  // 2-bit code + "is ACGT" plane: A=0 C=1 G=2 T=3
            const uint32_t one = (code != 0) & ((code & (code - 1)) == 0);
            const uint32_t two = (code == 2) ? 1u : (code == 4) ? 2u : (code == 8) ? 3u : 0u;
            a0 |= (two & 1u & one) << s; a1 |= ((two >> 1) & one) << s; a2 |= one << s;
          }
        }
        pl[0][j] = a0; pl[1][j] = a1; pl[2][j] = a2; pl[3][j] = a3;
        if (partial_code) {
          const int pos = atomicAdd(&amb_n[lane], 1);
          if (pos < AMB_CAP) { amb_w[lane][pos] = w4 * 4 + j; amb_p[lane][pos][0] = a0; amb_p[lane][pos][1] = a1; amb_p[lane][pos][2] = a2; amb_p[lane][pos][3] = a3; }
        }
      }
      uint4 *dst = tiles + ((size_t)(tile * W4 + w4) * P) * 64 + lane;
#pragma unroll
      for (int p = 0; p < P; p++) dst[(size_t)p * 64] = make_uint4(pl[p][0], pl[p][1], pl[p][2], pl[p][3]);
    }
  }
  partial[wv][lane] = valid; partial_acgt[wv][lane] = n_acgt;
  __syncthreads();
  if (wv == 0 && active && non_n_out) non_n_out[slot] = partial[0][lane] + partial[1][lane] + partial[2][lane] + partial[3][lane];
  // total the two-counter scan subtracts from: valid sites (default) or ACGT sites (--acgt) of the whole sequence
  if (wv == 0 && active && tot_out) tot_out[slot] = (P == 4) ? (partial[0][lane] + partial[1][lane] + partial[2][lane] + partial[3][lane])
                                                           : (partial_acgt[0][lane] + partial_acgt[1][lane] + partial_acgt[2][lane] + partial_acgt[3][lane]);
  if (wv == 0 && active && amb_out) {
    int *a = amb_out + (size_t)slot * AMB_ROW;
    a[0] = amb_n[lane];
    for (int k = 0; k < AMB_CAP; k++) {
      const bool have = k < amb_n[lane];
      a[1 + k] = have ? amb_w[lane][k] : 0;
      for (int pp = 0; pp < 4; pp++) a[12 + 4 * k + pp] = have ? (int)amb_p[lane][k][pp] : 0;
    }
  }
  if (bad) atomicOr(errflag, 1);
}

// Packed interchange form -> this context's planes.  The on-disk database (uvaia_amd/csrc/host/uvdb.h) always holds the four
// IUPAC planes; a default-mode context copies them as they are, an --acgt context re-codes them to (lo, hi, isACGT).  Also
// writes the per-reference total the two-counter scan subtracts from (valid sites / ACGT sites).  One block per tile.
template <int P>
__global__ __launch_bounds__(256) void import_tiles_kernel(const uint4 *src, int W4, uint4 *dst /* P == 4: may be NULL = planes are in place already */, long long tile_base,
                                                            int *__restrict__ tot_out)
{
  __shared__ int partial[4][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long tile = tile_base + blockIdx.x;
  const uint4 *t = src + (size_t)blockIdx.x * W4 * 4 * 64 + lane;
  uint4 *o = dst + (size_t)tile * W4 * P * 64 + lane;
  int tot = 0;
  for (int w4 = wv; w4 < W4; w4 += 4) {
    const uint4 pA = t[(size_t)(w4 * 4 + 0) * 64], pC = t[(size_t)(w4 * 4 + 1) * 64], pG = t[(size_t)(w4 * 4 + 2) * 64], pT = t[(size_t)(w4 * 4 + 3) * 64];
    if (P == 4) {
      if (dst) { o[(size_t)(w4 * 4 + 0) * 64] = pA; o[(size_t)(w4 * 4 + 1) * 64] = pC; o[(size_t)(w4 * 4 + 2) * 64] = pG; o[(size_t)(w4 * 4 + 3) * 64] = pT; }
#pragma unroll
      for (int j = 0; j < 4; j++) tot += __popc(u4c(pA, j) | u4c(pC, j) | u4c(pG, j) | u4c(pT, j));
    } else {
      uint32_t L[4], H[4], I[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint32_t a = u4c(pA, j), cc = u4c(pC, j), g = u4c(pG, j), tt = u4c(pT, j);
        const uint32_t par = a ^ cc ^ g ^ tt, three = (a & cc & (g | tt)) | (g & tt & (a | cc));
        I[j] = par & ~three; L[j] = (cc | tt) & I[j]; H[j] = (g | tt) & I[j];
        tot += __popc(I[j]);
      }
      o[(size_t)(w4 * 3 + 0) * 64] = make_uint4(L[0], L[1], L[2], L[3]);
      o[(size_t)(w4 * 3 + 1) * 64] = make_uint4(H[0], H[1], H[2], H[3]);
      o[(size_t)(w4 * 3 + 2) * 64] = make_uint4(I[0], I[1], I[2], I[3]);
    }
  }
  partial[wv][lane] = tot;
  __syncthreads();
  if (wv == 0) tot_out[tile * 64 + lane] = partial[0][lane] + partial[1][lane] + partial[2][lane] + partial[3][lane];
}

// Side rows and valid-site counts that arrive through uvaia_gpu_db_append_packed are external input: the replay indexes query
// planes with the listed word numbers.  A row that lists a word outside the alignment (or a negative count) is turned into
// "list incomplete" (count above AMB_CAP: the pair is rescanned densely, same result as a correct row); counts are clamped.
__global__ void sanitise_import_kernel(int *__restrict__ side_rows /* nullable */, int *__restrict__ non_n, long long n_slots, int n_words, int nchar)
{
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_slots) return;
  non_n[i] = min(max(non_n[i], 0), nchar);
  if (!side_rows) return;
  int *row = side_rows + (size_t)i * AMB_ROW;
  const int cnt = row[0];
  bool ok = cnt >= 0;
  for (int k = 0; k < AMB_CAP && k < cnt; k++) ok = ok && row[1 + k] >= 0 && row[1 + k] < n_words;
  if (!ok) { row[0] = AMB_CAP + 1; for (int k = 0; k < AMB_CAP; k++) row[1 + k] = 0; }
}

// Windowed search (host_window.inc): tiles of the interchange form that were staged as the file holds them -> tiles of the same form that
// hold the selected references only, in order.  Destination slot k = tile k / 64, lane k % 64 receives every 16-byte piece of staged slot
// sel[k] (sel == NULL: slot k), its valid-site count and its side row; lanes at and past n_ref are written as zero planes, zero count and
// zero side row, so a destination tile is complete whatever it held before.  One block per destination tile, lane = destination reference:
// a wave moves one plane of one word group per load, and with few exclusions consecutive lanes read consecutive 16-byte words of the same
// staged tile (the holes shift the run by a lane, a run that crosses a tile boundary continues in the next tile).  Side rows: one wave per
// reference, lane = int of the row, the reference's staged slot handed round by a shuffle.  sel[] was checked by the host against the
// staged tiles; nothing here depends on what the staged bytes hold.
__global__ __launch_bounds__(256) void select_tiles_kernel(const uint4 *__restrict__ src, const int *__restrict__ src_nonn, const int *__restrict__ src_side /* nullable */,
                                                            const int *__restrict__ sel /* nullable */, int n_ref, int W4,
                                                            uint4 *__restrict__ dst, int *__restrict__ dst_nonn, int *__restrict__ dst_side /* nullable, with src_side */)
{
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long k = (long long)blockIdx.x * 64 + lane;
  const bool active = k < n_ref;
  const int s = active ? (sel ? sel[k] : (int)k) : 0;
  const uint4 *t = src + (size_t)(s >> 6) * W4 * 4 * 64 + (s & 63);
  uint4 *o = dst + (size_t)blockIdx.x * W4 * 4 * 64 + lane;
  const int rows = W4 * 4;                             // (word group, plane) rows of 64 lanes
  for (int r = wv; r < rows; r += 4) o[(size_t)r * 64] = active ? ld_stream(t + (size_t)r * 64) : make_uint4(0u, 0u, 0u, 0u);
  if (wv == 0) dst_nonn[k] = active ? src_nonn[s] : 0;
  if (dst_side) {
    for (int i = wv; i < 64; i += 4) {
      const int si = __shfl(s, i);
      const long long ki = (long long)blockIdx.x * 64 + i;
      dst_side[(size_t)ki * AMB_ROW + lane] = ki < n_ref ? src_side[(size_t)si * AMB_ROW + lane] : 0;
    }
  }
}

// Append of staged lanes behind the references already resident (uvaia_gpu_db_append_staged, host_window.inc): destination slot
// slot0 + k, k in [0, n_ref), = tile (slot0 + k) / 64, lane (slot0 + k) % 64 of the resident store receives staged slot sel[k]
// (sel == NULL: slot k).  slot0 is any position: the first destination tile may hold resident references in the lanes below slot0 % 64,
// and a thread of such a lane stores nothing at all -- no plane word, count, total or side row -- so they survive untouched without a
// read-modify-write.  Lanes at and past slot0 + n_ref of the last tile are written as zero, as uvaia_gpu_db_export promises.  Selection,
// the re-coding of an --acgt context (P == 3, as import_tiles_kernel<3>, plus the four-plane image in `four` that the text is decoded
// from) and the totals are one pass: a wave loads the four planes of one word group, 64 lanes x 16 bytes each, and stores P of them.  With
// few exclusions consecutive lanes read consecutive 16-byte words of one staged tile, shifted against the destination lanes by
// (slot0 - first staged lane) % 64: a wave load is then two contiguous runs, the end of one staged tile's 1 KiB row and the start of the
// next tile's, whose other halves the neighbouring blocks read (no lane order to mend, so no LDS transpose), and the stores are whole
// 1 KiB rows but for the first tile's resident lanes.  One block per
// destination tile, tile_base = slot0 / 64.  Side rows as in select_tiles_kernel: one wave per reference.  sel[] was checked by the host.
template <int P>
__global__ __launch_bounds__(256) void append_lanes_kernel(const uint4 *__restrict__ src, const int *__restrict__ src_nonn, const int *__restrict__ src_side /* nullable */,
                                                            const int *__restrict__ sel /* nullable */, long long slot0, int n_ref, int W4,
                                                            uint4 *__restrict__ dst, uint4 *__restrict__ four /* P == 3 only, nullable */, long long tile_base,
                                                            int *__restrict__ dst_nonn, int *__restrict__ dst_side /* nullable, with src_side */, int *__restrict__ dst_tot)
{
  __shared__ int partial[4][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long tile = tile_base + blockIdx.x;
  const long long slot = tile * 64 + lane;
  const long long k = slot - slot0;
  const bool mine = k >= 0;                            // lanes below slot0 hold resident references
  const bool active = mine && k < n_ref;
  const int s = active ? (sel ? sel[k] : (int)k) : 0;
  const uint4 *t = src + (size_t)(s >> 6) * W4 * 4 * 64 + (s & 63);
  uint4 *o = dst + (size_t)tile * W4 * P * 64 + lane;
  uint4 *f = (P == 3 && four) ? four + (size_t)tile * W4 * 4 * 64 + lane : nullptr;
  int tot = 0;
  if (mine) for (int w4 = wv; w4 < W4; w4 += 4) {
    uint4 pA = make_uint4(0u, 0u, 0u, 0u), pC = pA, pG = pA, pT = pA;
    if (active) { pA = ld_stream(t + (size_t)(w4 * 4 + 0) * 64); pC = ld_stream(t + (size_t)(w4 * 4 + 1) * 64); pG = ld_stream(t + (size_t)(w4 * 4 + 2) * 64); pT = ld_stream(t + (size_t)(w4 * 4 + 3) * 64); }
    if (P == 4) {
      o[(size_t)(w4 * 4 + 0) * 64] = pA; o[(size_t)(w4 * 4 + 1) * 64] = pC; o[(size_t)(w4 * 4 + 2) * 64] = pG; o[(size_t)(w4 * 4 + 3) * 64] = pT;
#pragma unroll
      for (int j = 0; j < 4; j++) tot += __popc(u4c(pA, j) | u4c(pC, j) | u4c(pG, j) | u4c(pT, j));
    } else {
      uint32_t L[4], H[4], I[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint32_t a = u4c(pA, j), cc = u4c(pC, j), g = u4c(pG, j), tt = u4c(pT, j);
        const uint32_t par = a ^ cc ^ g ^ tt, three = (a & cc & (g | tt)) | (g & tt & (a | cc));
        I[j] = par & ~three; L[j] = (cc | tt) & I[j]; H[j] = (g | tt) & I[j];
        tot += __popc(I[j]);
      }
      o[(size_t)(w4 * 3 + 0) * 64] = make_uint4(L[0], L[1], L[2], L[3]);
      o[(size_t)(w4 * 3 + 1) * 64] = make_uint4(H[0], H[1], H[2], H[3]);
      o[(size_t)(w4 * 3 + 2) * 64] = make_uint4(I[0], I[1], I[2], I[3]);
      if (f) { f[(size_t)(w4 * 4 + 0) * 64] = pA; f[(size_t)(w4 * 4 + 1) * 64] = pC; f[(size_t)(w4 * 4 + 2) * 64] = pG; f[(size_t)(w4 * 4 + 3) * 64] = pT; }
    }
  }
  partial[wv][lane] = tot;
  __syncthreads();
  if (wv == 0 && mine) {
    dst_tot[slot] = partial[0][lane] + partial[1][lane] + partial[2][lane] + partial[3][lane];
    dst_nonn[slot] = active ? src_nonn[s] : 0;
  }
  if (dst_side) {
    for (int i = wv; i < 64; i += 4) {
      const int si = __shfl(s, i);
      const long long ki = tile * 64 + i - slot0;
      if (ki < 0) continue;
      dst_side[(size_t)(tile * 64 + i) * AMB_ROW + lane] = ki < n_ref ? src_side[(size_t)si * AMB_ROW + lane] : 0;
    }
  }
}

// The opposite of pack_refs_kernel<4>: the upper-case text of selected references out of tiles of the interchange form (four IUPAC
// planes).  One block per selected reference (index[] = positions in the batch, any order, repeats allowed: every row is independent),
// one thread per 16 sites = one half of an alignment word: eight neighbouring threads read the same 16-byte piece of each plane (one
// request), a wave reads eight pieces 4 KiB apart per plane and writes 1 KiB of contiguous text.  Per site the character is
// code[A | C << 1 | G << 2 | T << 3]; the empty set reads 'N' here, the sparse exception runs ('-', '?', 'X', 'O', '.') are the host's.
// Four sites at a time by iupac_text4 (iupac_decode.h, shared with the clusterer's whole-tile decode).  Sites at and beyond nchar are
// not written.
__global__ __launch_bounds__(256) void unpack_rows_kernel(const uint4 *__restrict__ tiles, int W4, int nchar, const int *__restrict__ index,
                                                           uint8_t *__restrict__ rows, size_t pitch /* a multiple of 16 */)
{
  const int r = index[blockIdx.x];
  const uint32_t *t = reinterpret_cast<const uint32_t *>(tiles + (size_t)(r >> 6) * W4 * 4 * 64 + (r & 63));
  uint8_t *row = rows + (size_t)blockIdx.x * pitch;
  const int n16 = (nchar + 15) >> 4;
  for (int k = threadIdx.x; k < n16; k += 256) {
    const int word = k >> 1, sh = (k & 1) * 16;
    const uint32_t *p = t + (size_t)(word >> 2) * (4 * 64 * 4) + (word & 3);      // plane A of the word; the planes of a word group are 64 uint4 apart
    const uint32_t a = p[0] >> sh, c = p[256] >> sh, g = p[512] >> sh, tt = p[768] >> sh;
    uint32_t out[4];
#pragma unroll
    for (int q = 0; q < 4; q++) out[q] = iupac_text4((a >> (4 * q)) & 15u, (c >> (4 * q)) & 15u, (g >> (4 * q)) & 15u, (tt >> (4 * q)) & 15u);
    const int site0 = k * 16;
    if (site0 + 16 <= nchar) *reinterpret_cast<uint4 *>(row + site0) = make_uint4(out[0], out[1], out[2], out[3]);
    else {
#pragma unroll
      for (int s = 0; s < 16; s++) if (site0 + s < nchar) row[site0 + s] = (uint8_t)(out[s >> 2] >> ((s & 3) * 8));
    }
  }
}

// ------------------------------------------------------------------------------------------------------------
// device: the column walk of create_query_indices (src/fastaseq.c:732-777) over the query rows
// ------------------------------------------------------------------------------------------------------------
// Per column of the trimmed window: the first usable character (a query is usable at a site when it is valid there, with --acgt when
// it is ACGT: src/fastaseq.c:746,753), whether a later usable one differs (the reference writes '#') and whether some query is not
// usable there (its miss[] flag).  The reference stops looking at a column once it is '#'; its miss[] is only read for columns that
// are not, so walking every query gives the same classes.  Two passes so that the rows of a batch are spread over the chip: blocks
// (x = 256 columns, y = 64 rows) reduce their rows in order, then one thread per column merges the row groups in order.
static __device__ __forceinline__ bool site_usable(uint8_t c, bool acgt)
{
  const uint8_t up = c & 0xDFu;
  if (acgt) return up == 'A' || up == 'C' || up == 'G' || up == 'T';
  return !(up == 'N' || up == 'X' || up == 'O' || c == '-' || c == '?' || c == '.');
}

__global__ __launch_bounds__(256) void query_columns_partial_kernel(const uint8_t *__restrict__ rows, size_t pitch, int n_rows, int lo, int hi, int acgt,
                                                                     uint8_t *__restrict__ part_first, uint8_t *__restrict__ part_flags, int nchar)
{
  const int col = lo + (int)(blockIdx.x * 256 + threadIdx.x);
  if (col >= hi) return;
  const int r0 = (int)blockIdx.y * 64, r1 = min(n_rows, r0 + 64);
  uint8_t first = 'N', flags = 0;                  // bit 0: two usable characters differ, bit 1: some query not usable
  for (int j = r0; j < r1; j++) {
    const uint8_t c = rows[(size_t)j * pitch + col];
    if (!site_usable(c, acgt != 0)) flags |= 2;
    else if (first == 'N') first = c;
    else if (first != c) flags |= 1;
  }
  part_first[(size_t)blockIdx.y * nchar + col] = first;
  part_flags[(size_t)blockIdx.y * nchar + col] = flags;
}

// merges the row groups of a batch (in order) into the running state of the column: state_first / state_flags carry over batches
__global__ __launch_bounds__(256) void query_columns_merge_kernel(const uint8_t *__restrict__ part_first, const uint8_t *__restrict__ part_flags, int n_groups, int lo, int hi,
                                                                   int nchar, uint8_t *__restrict__ state_first, uint8_t *__restrict__ state_flags)
{
  const int col = lo + (int)(blockIdx.x * 256 + threadIdx.x);
  if (col >= hi) return;
  uint8_t first = state_first[col], flags = state_flags[col];
  for (int g = 0; g < n_groups; g++) {
    const uint8_t f = part_first[(size_t)g * nchar + col];
    flags |= part_flags[(size_t)g * nchar + col];
    if (f != 'N') { if (first == 'N') first = f; else if (first != f) flags |= 1; }
  }
  state_first[col] = first; state_flags[col] = flags;
}
