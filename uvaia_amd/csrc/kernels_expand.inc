// kernels_expand.inc -- part of uvaia_gpu.hip (included there, not a translation unit of its own): the compact form of a packed database
// (version 2 of uvaia_amd/csrc/host/uvdb.h: a base row and, per reference, the 32-site words that differ from it) expanded, in a staging
// slot, into the dense tiles every other kernel takes.

// One block per tile, four waves.  Phase 1 writes the base into all 64 lanes of every [word group][plane] row: every lane stores the same
// 16 bytes, a wave store is one coalesced 1 KiB row.  After the block barrier (phase 2 rewrites dwords other waves of the block wrote)
// wave v takes lanes v, v + 4, ... of the tile; its 64 lanes take the reference's heads, 64 per round.  A head is
// first_word:16 | n_words:11 | literal:1 | code:4 (uvdb.h).  The payload of a literal head starts where the literal words of the heads
// before it end: an inclusive wave prefix sum over the literal word counts, the total carried from round to round.  A lane then writes its
// words with plain dword stores at (((w / 4) * 4 + p) * 64 + lane of the reference) * 16 + (w % 4) * 4 within the tile: records never
// overlap and a reference's words belong to its lane slot alone, so there is no atomic, no LDS transpose and no read-modify-write.  A
// long fill is looped by its one lane: rare (a wholly unknown row), and the stores of the other lanes of the round overlap it.
// The lanes past a file's last reference are encoded as all-zero rows, so nothing here knows where a file ends.
// The host has checked every index entry and head (uvdb_open); the kernel does not rely on it: head positions are clamped to the n_heads
// records that were copied, literal words to n_lit_words, and every store is bounded by W4.  head_idx / lit_idx: 64 * gridDim.x + 1
// offsets as the file holds them; the records copied start at the first one's.
__global__ __launch_bounds__(256) void expand_tiles_kernel(const uint4 *__restrict__ base, const unsigned long long *__restrict__ head_idx, const uint32_t *__restrict__ heads,
                                                            unsigned long long n_heads, const unsigned long long *__restrict__ lit_idx, const uint32_t *__restrict__ lits,
                                                            unsigned long long n_lit_words, int W4, uint4 *__restrict__ dst)
{
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint4 *tile = dst + (size_t)blockIdx.x * W4 * 4 * 64;
  const int rows = W4 * 4;
  for (int r = wv; r < rows; r += 4) tile[(size_t)r * 64 + lane] = base[r];
  __syncthreads();
  uint32_t *tw = reinterpret_cast<uint32_t *>(tile);
  const uint32_t n_words = (uint32_t)W4 * 4;
  const unsigned long long h0 = head_idx[0], l0 = lit_idx[0];
  for (int i = wv; i < 64; i += 4) {
    const size_t g = (size_t)blockIdx.x * 64 + i;
    const unsigned long long hb = min(head_idx[g] - h0, n_heads), he = min(head_idx[g + 1] - h0, n_heads);
    unsigned long long carry = lit_idx[g] - l0;                     // literal words in front of this round's
    for (unsigned long long h = hb; h < he; h += 64) {
      const bool have = h + lane < he;
      const uint32_t head = have ? heads[h + lane] : 0u;
      const uint32_t first = head >> 16, nw = (head >> 5) & 0x7FFu, code = head & 15u;
      const bool literal = (head >> 4) & 1u;
      uint32_t incl = literal ? nw : 0u;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) { const uint32_t up = __shfl_up(incl, d); if (lane >= d) incl += up; }
      const unsigned long long mine = carry + incl - (literal ? nw : 0u);
      carry += __shfl(incl, 63);
      uint32_t *o = tw + (size_t)i * 4;
      for (uint32_t q = 0; q < nw; q++) {
        const uint32_t w = first + q;
        if (w >= n_words) break;
        uint32_t v[4];
        if (literal) {
          if (mine + q >= n_lit_words) break;
          const uint4 x = *reinterpret_cast<const uint4 *>(lits + (mine + q) * 4);
          v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
        } else {
#pragma unroll
          for (int p = 0; p < 4; p++) v[p] = ((code >> p) & 1u) ? 0xFFFFFFFFu : 0u;
        }
        uint32_t *ow = o + (size_t)(w >> 2) * (4 * 64 * 4) + (w & 3);
#pragma unroll
        for (int p = 0; p < 4; p++) ow[(size_t)p * 256] = v[p];
      }
    }
  }
}

// Side rows of staged tiles, as side_rows_canonical_kernel writes those of the resident database -- the partially ambiguous words of a
// reference in ascending order, the first AMB_CAP listed with their planes, the count as the total -- and the whole row of AMB_ROW ints:
// what lies behind the listed planes is zero, as in the rows a dense file holds.  One wave per tile, lane = slot.
__global__ __launch_bounds__(64) void side_rows_staged_kernel(const uint4 *__restrict__ tiles, int W4, int *__restrict__ side)
{
  const uint4 *t = tiles + (size_t)blockIdx.x * W4 * 4 * 64 + threadIdx.x;
  int *row = side + ((size_t)blockIdx.x * 64 + threadIdx.x) * AMB_ROW;
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
  for (int k = 12 + 4 * AMB_CAP; k < AMB_ROW; k++) row[k] = 0;
}
