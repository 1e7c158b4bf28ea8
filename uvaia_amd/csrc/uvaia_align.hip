// uvaia_align.hip -- MI355X (gfx950 / CDNA4) gap-affine wavefront aligner behind include/uvaia_align.h.
//
// What it replaces in the reference (paths under /root/reference): the OpenMP loop of src/align.c:224-233 over
// align_query (src/align.c:357-364) and update_query_aligned (src/align.c:366-390), and the per-thread WFA aligners of
// new_queue (src/align.c:286-313).  The WFA library is an absent submodule; the algorithm is the published one
// (Marco-Sola et al. 2021) as oracle/wfa_oracle.h states it, and this file reproduces that statement bit for bit.
//
// Design ("uvaialign"):
//   * one block of four waves per query, persistent: a block takes the next query from an atomic counter until none is left.
//     A query is a chain of thousands of dependent steps (one per score); N-rich sequences (the normal SARS-CoV-2 case) make
//     the wavefronts 1 000-2 000 diagonals wide for most of them, so a step has work for 256 lanes and one barrier.
//   * lane = diagonal.  A step computes I, D, M of 256 diagonals at a time from the wavefronts of score - e, score - o - e,
//     score - x, extends M along the diagonal in registers (eight characters per lane in one unaligned 8-byte compare; longer
//     runs by the whole wave, 1 024 characters per round trip) and stores M once.  Reference and queries are read through L2.
//     A wave takes its diagonals two groups of 64 at a time and asks for the characters of both before it compares either.
//   * the wavefronts a step reads are those of the last few steps: they stay in LDS (16-bit offsets, up to 2 560 diagonals) and
//     the stores to the history in memory are not waited for; wider wavefronts and unusual penalties fall back to memory.
//     The step is compiled twice: the usual one, whose wavefront and sources are all in LDS, carries none of the bookkeeping of
//     the fallbacks (the kernel is bound by instruction issue: what a step executes besides its cells is what it costs).
//   * what is kept for the backtrace is 5 bytes per cell, not 12: the M offset and one provenance byte (which of the five
//     predecessors gave the maximum, in the backtrace's tie order; whether the I and the D cell extend or open).  I and D
//     offsets only feed the next e scores and live in a ring chunk.  A ring of the last 64 headers lives in LDS.
//   * wavefront memory comes in chunks from a pool shared by the blocks in flight (a query takes what its score needs: 2 MB
//     to more than 1 GB); a query that finds the pool empty is flagged and run again in a later, less crowded pass.
//   * the backtrace runs on wave 0 right after the last step and writes the projected row (ref_len characters) directly:
//     match runs are copied 64 characters at a time, runs of mismatches (N runs) are taken 63 steps per round trip.
//   * the characters the projection drops (insertion runs) are reported on request (uvaia_align_set_insertions): the kernel's body,
//     wfa_align_body.inc, is compiled a second time as wfa_align_insertions_kernel, whose backtrace writes one record per run.
//   * what a finished row differs from the reference by (substitutions, deletion runs, per-row counts) is derived from the rows where they
//     lie, on request (uvaia_align_set_variants, uvaia_align_variants_of): three small kernels of their own, align_variants.inc.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/uvaia_align.h"
#include "rows_block.h"

// build-time shape (tools/ab_align.sh measures variants): groups of 64 diagonals a wave has in flight, waves per block
#ifndef WFA_GROUP
#define WFA_GROUP 2
#endif
#ifndef WFA_NW
#define WFA_NW 4
#endif

namespace {

constexpr int WFA_NULL = -10;            // offset of a diagonal a wavefront does not hold (oracle/wfa_oracle.c)
constexpr int NW = WFA_NW;               // waves per block = per query
constexpr int TPB = 64 * NW;
constexpr int RING = 64;                 // scores whose headers stay in LDS; penalties are below this
constexpr int HDR_INTS = 8;
constexpr int HDR_PAGE_SCORES = 2048;    // headers of all scores live in pages of the query's own memory (the backtrace reads them)
constexpr int MAX_HDR_PAGES = 256;
constexpr int MAX_OWN = 512;             // chunks a query may hold on top of the block's two permanent ones
constexpr int WL = 2560;                 // widest wavefront kept in LDS (16-bit offsets + 16)
constexpr int RM = 5, RID = 2;           // LDS slots: M wavefronts of the last RM steps, I and D of the last RID
enum { ST_OK = 0, ST_OVERFLOW = 1, ST_MAXSCORE = 2, ST_BACKTRACE = 3, ST_TOOWIDE = 4, ST_HDRPAGES = 5, ST_INSFULL = 6 };
enum { C_DEL_EXT = 0, C_DEL_OPEN = 1, C_INS_EXT = 2, C_INS_OPEN = 3, C_MISMATCH = 4, C_I_EXT = 8, C_D_EXT = 16 };

struct WfaParams { int x, oe, e, min_wf_len, max_dist_thr, max_score, g; };
template <bool B> struct BoolTag { static constexpr bool value = B; };

// Workspace: chunks of 2^chunk_log2 words handed out from a stack under a spin lock (one thread of a block at a time, the others
// wait at a barrier; a query takes a chunk every few hundred thousand cells).  Block b owns chunks 2b (first history chunk) and
// 2b + 1 (ring of the I and D wavefronts) for the whole launch.
struct PoolCtl { int lock, top, n_chunks, chunk_log2; };

// Header of the wavefronts of one score.  M, I and D share their limits (the reduction trims M and hands its limits to I and D).
// flags bit 0 = M exists, bit 1 = I, bit 2 = D.  off16 / id16: where the arrays start, in units of 16 words from the pool's base:
// history = M offsets (w words, padded to 16) followed by one provenance byte per cell; I and D (w16 words each) in the ring chunk.
struct Hdr { int lo, hi, lo_base, flags; uint32_t off16; int w; uint32_t id16; int res; };   // res: 1 + number of the step if its wavefronts went to LDS, else 0

__device__ __forceinline__ int rfl(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int w16_of(int w) { return (w + 15) & ~15; }
__device__ __forceinline__ bool in_range(const Hdr &h, int bit, int k) { return ((h.flags >> bit) & 1) && k >= h.lo && k <= h.hi; }
__device__ __forceinline__ int dist_to_end(int plen, int tlen, int offset, int k) { return max(plen - (offset - k), tlen - offset); }

__device__ __forceinline__ int matching_prefix8(const uint8_t *a, const uint8_t *b)
{ // leading bytes (0..8) on which the two strings agree; the compiler picks the load width it may use for unaligned addresses
  unsigned long long x, y;
  __builtin_memcpy(&x, a, 8); __builtin_memcpy(&y, b, 8);
  const unsigned long long d = x ^ y;
  return d ? (int)(__builtin_ctzll(d) >> 3) : 8;
}

// minimum over the wave by DPP (row shifts, then row broadcasts): six VALU steps, no trip through the LDS crossbar
__device__ __forceinline__ int wave_min_dpp(int v)
{
  const int big = 0x7fffffff;
  v = min(v, __builtin_amdgcn_update_dpp(big, v, 0x111, 0xF, 0xF, false));    // row_shr:1
  v = min(v, __builtin_amdgcn_update_dpp(big, v, 0x112, 0xF, 0xF, false));    // row_shr:2
  v = min(v, __builtin_amdgcn_update_dpp(big, v, 0x114, 0xF, 0xF, false));    // row_shr:4
  v = min(v, __builtin_amdgcn_update_dpp(big, v, 0x118, 0xF, 0xF, false));    // row_shr:8  -> lane 15 of every row holds the row's minimum
  v = min(v, __builtin_amdgcn_update_dpp(big, v, 0x142, 0xA, 0xF, false));    // row_bcast:15 into rows 1 and 3
  v = min(v, __builtin_amdgcn_update_dpp(big, v, 0x143, 0xC, 0xF, false));    // row_bcast:31 into rows 2 and 3
  return __builtin_amdgcn_readlane(v, 63);
}

// barrier for steps whose wavefronts are exchanged through LDS only: the stores to the history in memory stay in flight
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__device__ __forceinline__ void pool_lock(PoolCtl *c) { while (atomicCAS(&c->lock, 0, 1) != 0) __builtin_amdgcn_s_sleep(4); __threadfence(); }
__device__ __forceinline__ void pool_unlock(PoolCtl *c) { __threadfence(); atomicExch(&c->lock, 0); }

// Where the insertion records of a launch go (the kernel compiled with INS): `cap` records of {query, ref_pos, seq_pos, length}, the
// number of records asked for so far (it goes on counting when the buffer is full) and the number of runs of every query.
static_assert(sizeof(uvaia_align_insertion) == sizeof(int4), "a record is one 16-byte store");
struct InsOut { int4 *rec; int cap; int *n_rec; int *runs; };

// The aligner proper is wfa_align_body.inc, compiled twice: wfa_align_kernel, and wfa_align_insertions_kernel, which also reports the insertion
// runs the projection drops.  Nothing of the second is in the first.
__global__ __launch_bounds__(TPB) void wfa_align_kernel(const uint8_t *__restrict__ ref, int plen, const uint8_t *__restrict__ seqs, const long long *__restrict__ seq_off,
                                                         const int *__restrict__ todo, int n_todo, uint8_t *__restrict__ aln, size_t aln_pitch, int *__restrict__ score_out,
                                                         int *__restrict__ status_out, unsigned long long *__restrict__ cells_out, uint32_t *__restrict__ pool,
                                                         PoolCtl *ctl, int *stack, int *next_query, WfaParams P)
{
  constexpr bool INS = false;
  const InsOut ins{nullptr, 0, nullptr, nullptr};
#include "wfa_align_body.inc"
}

__global__ __launch_bounds__(TPB) void wfa_align_insertions_kernel(const uint8_t *__restrict__ ref, int plen, const uint8_t *__restrict__ seqs, const long long *__restrict__ seq_off,
                                                                    const int *__restrict__ todo, int n_todo, uint8_t *__restrict__ aln, size_t aln_pitch, int *__restrict__ score_out,
                                                                    int *__restrict__ status_out, unsigned long long *__restrict__ cells_out, uint32_t *__restrict__ pool,
                                                                    PoolCtl *ctl, int *stack, int *next_query, WfaParams P, InsOut ins)
{
  constexpr bool INS = true;
#include "wfa_align_body.inc"
}

// The bases of the insertion runs: record r (sorted by the host) takes rec[r].w characters of its query from seq_pos on and puts them at
// at[r] of one contiguous buffer.  One wave per record; the host has checked every record against its query's length.
__global__ __launch_bounds__(256) void insertion_bases_kernel(const int4 *__restrict__ rec, const long long *__restrict__ at, int n_rec, const uint8_t *__restrict__ seqs,
                                                              const long long *__restrict__ seq_off, uint8_t *__restrict__ bases)
{
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= n_rec) return;
  const int4 c = rec[r];
  const uint8_t *src = seqs + seq_off[c.x] + c.z;
  uint8_t *dst = bases + at[r];
  for (int j = lane; j < c.w; j += 64) dst[j] = src[j];
}

// What a query is going to cost, roughly: every site that is no A, C, G or T is a mismatch against the reference (4 each, and N runs
// are what makes scores of tens of thousands), every character of length difference a gap extension.  The blocks are persistent and
// take the next query when they finish one, so the last queries to start decide how long the launch's tail is: the dearer half of
// the pool is started first, in the order it came (all of the dearest at once would also want all of the workspace at once), then
// the cheaper half in descending order of the estimate; a small pool is in descending order throughout.  One block per query.
__global__ __launch_bounds__(256) void expected_cost_kernel(const uint8_t *__restrict__ seqs, const long long *__restrict__ seq_off, int plen, int n, int *__restrict__ cost)
{
  __shared__ int part[4];
  const int q = blockIdx.x;
  if (q >= n) return;
  const uint8_t *t = seqs + seq_off[q];
  const int tlen = (int)(seq_off[q + 1] - seq_off[q]);
  int c = 0;
  for (int i = threadIdx.x; i < tlen; i += 256) { const uint8_t ch = t[i] & 0xDF; c += !(ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T'); }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) cost[q] = 4 * (part[0] + part[1] + part[2] + part[3]) + 2 * abs(tlen - plen);
}

#include "align_variants.inc"

thread_local std::string g_align_open_error;

}  // namespace

// ---- host side.  Device memory, events and the stream are the move-only handles of host_owners.h; a failed HIP call goes through hip_failed.
struct uvaia_aligner;
namespace { int hip_failed(uvaia_aligner *a, hipError_t e, const char *call, const char *file, int line); }
#include <memory>
#include "host_owners.h"

// Members are destroyed last to first: the stream comes first so that it outlives every buffer and event that work queued on it may still
// name (uvaia_align_close has waited for it by then).
struct uvaia_aligner {
  Stream stream;
  Event ev_a, ev_b;
  int device = 0;
  int plen = 0;
  WfaParams P{};
  DevBuf<uint8_t> d_ref, d_seqs;
  // per query of the pool, n_cap of each: offsets (one more), aligned rows, scores, status, the queries of a later pass, the pool's queries the dearest first
  DevBuf<long long> d_off; DevBuf<uint8_t> d_aln; DevBuf<int> d_score, d_status, d_todo, d_order;
  DevBuf<int> d_next;
  DevBuf<unsigned long long> d_cells;
  // wavefront memory: n_chunks chunks of 2^chunk_log2 words, the control block and the stack of free chunks.  n_chunks is set last and
  // says that all of it is there: a workspace that could not be built is empty
  struct Workspace {
    DevBuf<uint32_t> pool; DevBuf<PoolCtl> ctl; DevBuf<int> stack;
    int n_chunks = 0, chunk_log2 = 0;
    std::vector<int> h_stack;
  } ws;
  size_t n_cap = 0, workspace_request = 0;
  int n = 0, max_blocks = 0, passes = 0;
  bool ran = false;
  unsigned long long cells = 0;
  double kernel_ms = 0;
  std::vector<char> h_bytes; std::vector<long long> h_off;
  // insertion runs (uvaia_align_set_insertions): the record buffer of a launch, its counter, the runs of every query; the sorted records,
  // where their bases go and the bases.  On the host: the records of the last run, sorted by (query, ref_pos), and their bases.
  struct Insertions {
    bool on = false, done = false;
    size_t cap_request = 0;
    DevBuf<int4> rec, sorted; DevBuf<int> n_rec, runs; DevBuf<long long> at; DevBuf<uint8_t> bases;
    std::vector<uvaia_align_insertion> h_rec; std::vector<char> h_bases;
  } ins;
  // substitutions, deletions and per-row counts (uvaia_align_set_variants, uvaia_align_variants_of): the last answer stays on the device
  // until it is fetched -- two int4 of counts per row, the rows' offsets into the records, the records; `rows` holds what variants_of copies in
  struct Variants {
    bool on = false, done = false, from_run = false;
    int n_rows = 0;
    long long total = 0;
    double ms = 0;
    DevBuf<uint8_t> rows; DevBuf<int4> qc, rec; DevBuf<long long> off;
    Event e0, e1, e2, e3;
  } var;
  std::string err;
};

namespace {

int afail(uvaia_aligner *a, int code, const char *fmt, ...)
{
  char buf[512];
  va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
  if (a) a->err = buf; else g_align_open_error = buf;
  return code;
}

// (a is null while uvaia_align_open builds the aligner: the message goes where uvaia_align_last_error(NULL) finds it)
int hip_failed(uvaia_aligner *a, hipError_t e, const char *call, const char *file, int line)
{ return afail(a, e == hipErrorOutOfMemory ? UVAIA_ALIGN_ENOMEM : UVAIA_ALIGN_EHIP, "%s failed: %s (%s:%d)", call, hipGetErrorString(e), file, line); }

// room for a pool of n queries and `bytes` characters; the six per-query arrays grow as a group
int ensure_pool(uvaia_aligner *a, size_t bytes, int n)
{
  if (bytes + 512 > a->d_seqs.cap) if (int rc = a->d_seqs.reserve(a, std::max<size_t>(bytes + 512, 1u << 20) * 5 / 4)) return rc;
  if ((size_t)n > a->n_cap) {
    const size_t cap = std::max<size_t>((size_t)n * 5 / 4, 256);
    a->n_cap = 0;
    int rc;
    if ((rc = a->d_off.reserve(a, cap + 1)) || (rc = a->d_aln.reserve(a, cap * ((size_t)a->plen + 1))) || (rc = a->d_score.reserve(a, cap)) ||
        (rc = a->d_status.reserve(a, cap)) || (rc = a->d_todo.reserve(a, cap)) || (rc = a->d_order.reserve(a, cap))) return rc;
    a->n_cap = cap;
  }
  return 0;
}

// The workspace: with workspace_bytes == 0 it starts at 4 GB (a small job should not pay for mapping 200 GB) and grows by a factor
// of four, up to three quarters of the free device memory, whenever a pass leaves queries that found the pool empty.
int ensure_pool_memory(uvaia_aligner *a, bool grow, bool *grew)
{
  uvaia_aligner::Workspace &w = a->ws;
  if (grew) *grew = false;
  if (w.n_chunks && !grow) return 0;
  // a chunk holds the ring of I and D wavefronts (e + 2 pairs of the widest wavefront, at most all plen + tlen + 1 diagonals of a
  // query of up to 1.5 reference lengths, src/align.c:199) and serves as the unit the queries' histories grow by
  const unsigned long long widest = (unsigned long long)a->plen * 5 / 2 + 64;
  int lg = 19;
  while ((1ull << lg) < (unsigned long long)(a->P.e + 2) * 2ull * widest) lg++;
  if (lg > 28) return afail(a, UVAIA_ALIGN_EINVAL, "reference of %d sites is too long for the wavefront workspace", a->plen);
  const size_t chunk_bytes = (size_t)4 << lg, have = (size_t)w.n_chunks * chunk_bytes;
  if (w.n_chunks && a->workspace_request) return 0;                 // a workspace of a given size does not grow
  size_t free_b = 0, total_b = 0;
  HIPCHK(a, hipMemGetInfo(&free_b, &total_b));
  const size_t cap = std::min((free_b + have) / 4 * 3, (size_t)0xffffffffull * 64);   // array positions are kept in units of 64 bytes in 32 bits
  size_t want = a->workspace_request ? std::min(a->workspace_request, (size_t)0xffffffffull * 64) : std::min(cap, w.n_chunks ? have * 4 : std::max((size_t)4 << 30, 8 * chunk_bytes));
  if (w.n_chunks && want <= have) return 0;                         // already as large as it gets
  size_t n_chunks = want / chunk_bytes;
  if (n_chunks < 3) return afail(a, UVAIA_ALIGN_ENOMEM, "workspace of %zu bytes is below three chunks of %zu bytes", want, chunk_bytes);
  if (w.n_chunks) HIPCHK(a, hipStreamSynchronize(a->stream));
  w = uvaia_aligner::Workspace();                                   // the old one goes before the new one is asked for
  int rc;
  if ((rc = w.pool.reserve(a, n_chunks << lg)) || (rc = w.ctl.reserve(a, 1)) || (rc = w.stack.reserve(a, n_chunks))) { w = uvaia_aligner::Workspace(); return rc; }
  w.h_stack.resize(n_chunks);
  w.chunk_log2 = lg; w.n_chunks = (int)n_chunks;
  if (grew) *grew = true;
  return 0;
}

// The kernel over all queries of the pool, then again over those that found the workspace empty, until none is left.
int run_passes(uvaia_aligner *a)
{
  int n_todo = a->n;
  int blocks = std::max(1, std::min(std::min(n_todo, a->max_blocks), a->ws.n_chunks / 3));
  const int *todo = a->d_order;                                       // the first launch: every query of the pool, the dearest first
  std::vector<int> status((size_t)a->n), list, todo_list;             // todo_list empty: all queries of the pool
  // insertion records: the buffer of a launch is read and emptied after every pass; a query that found it full (ST_INSFULL) is run again
  // like one that found the workspace empty, its records of this pass are dropped and the buffer grows to what the counts of such queries say
  uvaia_aligner::Insertions &I = a->ins;
  std::vector<int> runs;
  std::vector<uvaia_align_insertion> got;
  size_t ins_cap = 0;
  if (I.on) {
    I.h_rec.clear();
    ins_cap = std::min<size_t>(I.cap_request ? I.cap_request : std::max<size_t>(65536, (size_t)a->n * 8), 0x7fffffff);
    int rc;
    if ((rc = I.rec.reserve(a, ins_cap)) || (rc = I.n_rec.reserve(a, 1)) || (rc = I.runs.reserve(a, a->n_cap))) return rc;
    runs.resize((size_t)a->n);
  }
  for (;;) {
    // every block keeps two chunks for the whole launch; the rest of the pool is what the queries in flight share
    const PoolCtl ctl{0, a->ws.n_chunks - 2 * blocks, a->ws.n_chunks, a->ws.chunk_log2};
    for (int i = 0; i < ctl.top; i++) a->ws.h_stack[(size_t)i] = 2 * blocks + i;
    HIPCHK(a, hipMemcpyAsync(a->ws.ctl, &ctl, sizeof ctl, hipMemcpyHostToDevice, a->stream));
    if (ctl.top > 0) HIPCHK(a, hipMemcpyAsync(a->ws.stack, a->ws.h_stack.data(), (size_t)ctl.top * sizeof(int), hipMemcpyHostToDevice, a->stream));
    HIPCHK(a, hipMemsetAsync(a->d_next, 0, sizeof(int), a->stream));
    HIPCHK(a, hipStreamSynchronize(a->stream));                     // (ctl is on the stack of this function)
    if (I.on) {
      HIPCHK(a, hipMemsetAsync(I.n_rec, 0, sizeof(int), a->stream));
      hipLaunchKernelGGL(wfa_align_insertions_kernel, dim3((unsigned)blocks), dim3(TPB), 0, a->stream, a->d_ref, a->plen, a->d_seqs, a->d_off, todo, n_todo, a->d_aln, (size_t)a->plen + 1,
                         a->d_score, a->d_status, a->d_cells, a->ws.pool, a->ws.ctl, a->ws.stack, a->d_next, a->P, InsOut{I.rec, (int)ins_cap, I.n_rec, I.runs});
    } else
      hipLaunchKernelGGL(wfa_align_kernel, dim3((unsigned)blocks), dim3(TPB), 0, a->stream, a->d_ref, a->plen, a->d_seqs, a->d_off, todo, n_todo, a->d_aln, (size_t)a->plen + 1,
                         a->d_score, a->d_status, a->d_cells, a->ws.pool, a->ws.ctl, a->ws.stack, a->d_next, a->P);
    HIPCHK(a, hipGetLastError());
    a->passes++;
    HIPCHK(a, hipMemcpyAsync(status.data(), a->d_status, (size_t)a->n * sizeof(int), hipMemcpyDeviceToHost, a->stream));
    HIPCHK(a, hipStreamSynchronize(a->stream));
    if (I.on) {
      int asked = 0;
      HIPCHK(a, hipMemcpyAsync(&asked, I.n_rec, sizeof(int), hipMemcpyDeviceToHost, a->stream));
      HIPCHK(a, hipMemcpyAsync(runs.data(), I.runs, (size_t)a->n * sizeof(int), hipMemcpyDeviceToHost, a->stream));
      HIPCHK(a, hipStreamSynchronize(a->stream));
      if (asked < 0) return afail(a, UVAIA_ALIGN_ESTATE, "more insertion runs in one pass than the counter holds");
      got.resize(std::min((size_t)asked, ins_cap));
      if (!got.empty()) HIPCHK(a, hipMemcpy(got.data(), I.rec, got.size() * sizeof(uvaia_align_insertion), hipMemcpyDeviceToHost));
      for (const uvaia_align_insertion &r : got) {
        if (r.query < 0 || r.query >= a->n) return afail(a, UVAIA_ALIGN_ESTATE, "insertion record of sequence %d, which the pool does not hold", r.query);
        if (status[(size_t)r.query] == ST_OK) I.h_rec.push_back(r);       // (what a query that is run again left is dropped here)
      }
    }
    list.clear();
    int n_over = 0;
    long long ins_need = 0;
    auto look = [&](int i) -> int {
      if (status[(size_t)i] == ST_OVERFLOW) { list.push_back(i); n_over++; }
      else if (status[(size_t)i] == ST_INSFULL) { list.push_back(i); ins_need += runs[(size_t)i]; }
      else if (status[(size_t)i] == ST_MAXSCORE) return afail(a, UVAIA_ALIGN_EINVAL, "sequence %d: alignment score above %d, the size of the reference's score table", i, a->P.max_score);
      else if (status[(size_t)i] == ST_HDRPAGES) return afail(a, UVAIA_ALIGN_EINVAL, "sequence %d: alignment score above %d, the most this aligner keeps score headers for (%d pages of %d scores)", i, MAX_HDR_PAGES * HDR_PAGE_SCORES - 1, MAX_HDR_PAGES, HDR_PAGE_SCORES);
      else if (status[(size_t)i] == ST_TOOWIDE) return afail(a, UVAIA_ALIGN_EINVAL, "sequence %d: a wavefront wider than the workspace's chunks hold (%zu bytes each)", i, (size_t)4 << a->ws.chunk_log2);
      else if (status[(size_t)i] != ST_OK) return afail(a, UVAIA_ALIGN_ESTATE, "sequence %d: inconsistent backtrace", i);
      return 0;
    };
    // (the status array holds what the last kernel to run a query left: only the queries of this launch are looked at)
    if (todo_list.empty()) { for (int i = 0; i < a->n; i++) { const int rc = look(i); if (rc) return rc; } }
    else for (int i : todo_list) { const int rc = look(i); if (rc) return rc; }
    if (list.empty()) break;
    bool grew = false;                                             // queries found the pool empty: a workspace of the library's choosing grows first, ...
    if (n_over) {
      { const int rc = ensure_pool_memory(a, true, &grew); if (rc) return rc; }
      if (!grew) {                                                 // ... then fewer queries go in flight
        if (blocks == 1) return afail(a, UVAIA_ALIGN_ENOMEM, "sequence %d needs more than the whole workspace (%zu bytes) for its wavefronts", list[0], ((size_t)a->ws.n_chunks * 4) << a->ws.chunk_log2);
        blocks = std::max(1, std::min((int)list.size(), blocks / 4));
      }
    } else blocks = std::max(1, std::min((int)list.size(), blocks));  // only the record buffer was short
    if (ins_need > (long long)ins_cap) {                           // every query that found the record buffer full finds room for all its runs
      if (ins_need > 0x7fffffffLL) return afail(a, UVAIA_ALIGN_ENOMEM, "%lld insertion runs are more than one record buffer holds", ins_need);
      ins_cap = (size_t)ins_need;
      if (int rc = I.rec.reserve(a, ins_cap)) return rc;           // (the stream is idle: every pass ends with a wait for it)
    }
    todo_list = list;
    HIPCHK(a, hipMemcpyAsync(a->d_todo, todo_list.data(), todo_list.size() * sizeof(int), hipMemcpyHostToDevice, a->stream));
    HIPCHK(a, hipStreamSynchronize(a->stream));
    todo = a->d_todo; n_todo = (int)todo_list.size();
    if (grew) blocks = std::max(1, std::min(std::min(n_todo, a->max_blocks), a->ws.n_chunks / 3));
  }
  return 0;
}

// The records of a completed run in their order -- by query, then by ref_pos -- and their bases, gathered on the device from the aligner's
// own copy of the pool into one buffer (the caller may have no query text: uvaia_align_load_device).
int gather_insertions(uvaia_aligner *a)
{
  uvaia_aligner::Insertions &I = a->ins;
  std::sort(I.h_rec.begin(), I.h_rec.end(), [](const uvaia_align_insertion &x, const uvaia_align_insertion &y) { return x.query != y.query ? x.query < y.query : x.ref_pos < y.ref_pos; });
  const size_t n = I.h_rec.size();
  std::vector<long long> at(n + 1, 0);
  for (size_t r = 0; r < n; r++) {     // the gather reads what the records say: they are checked against the pool first
    const uvaia_align_insertion &c = I.h_rec[r];
    const long long len = a->h_off[(size_t)c.query + 1] - a->h_off[(size_t)c.query];
    if (c.ref_pos < 0 || c.ref_pos > a->plen || c.seq_pos < 0 || c.length < 1 || (long long)c.seq_pos + c.length > len || (r > 0 && I.h_rec[r - 1].query == c.query && I.h_rec[r - 1].ref_pos == c.ref_pos))
      return afail(a, UVAIA_ALIGN_ESTATE, "sequence %d: inconsistent insertion record (%d bases at site %d, from character %d of %lld)", c.query, c.length, c.ref_pos, c.seq_pos, len);
    at[r + 1] = at[r] + c.length;
  }
  I.h_bases.assign((size_t)at[n], 0);
  if (!n) return 0;
  if (n > 0x7fffffff) return afail(a, UVAIA_ALIGN_ENOMEM, "%zu insertion runs are more than one gather takes", n);
  int rc;
  if ((rc = I.sorted.reserve(a, n)) || (rc = I.at.reserve(a, n)) || (rc = I.bases.reserve(a, (size_t)at[n]))) return rc;
  HIPCHK(a, hipMemcpyAsync(I.sorted, I.h_rec.data(), n * sizeof(uvaia_align_insertion), hipMemcpyHostToDevice, a->stream));
  HIPCHK(a, hipMemcpyAsync(I.at, at.data(), n * sizeof(long long), hipMemcpyHostToDevice, a->stream));
  hipLaunchKernelGGL(insertion_bases_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, a->stream, I.sorted, I.at, (int)n, a->d_seqs, a->d_off, I.bases);
  HIPCHK(a, hipGetLastError());
  HIPCHK(a, hipMemcpyAsync(I.h_bases.data(), I.bases, (size_t)at[n], hipMemcpyDeviceToHost, a->stream));
  HIPCHK(a, hipStreamSynchronize(a->stream));        // (at is on the stack of this function)
  return 0;
}

// The three passes of align_variants.inc over n rows on the device.  Only the number of records comes to the host between the second and
// the third, to size the record buffer.
int run_variants(uvaia_aligner *a, const uint8_t *d_rows, size_t pitch, int n, bool from_run)
{
  uvaia_aligner::Variants &V = a->var;
  V.done = false; V.from_run = from_run; V.n_rows = 0; V.total = 0;
  if (n > 0) {
    int rc;
    if ((rc = V.qc.reserve(a, 2 * (size_t)n)) || (rc = V.off.reserve(a, (size_t)n + 1)) || (rc = V.e0.make(a)) || (rc = V.e1.make(a)) || (rc = V.e2.make(a)) || (rc = V.e3.make(a))) return rc;
    const unsigned blocks = (unsigned)(((size_t)n + 3) / 4);
    long long total = 0;
    float ms = 0, ms_emit = 0;
    HIPCHK(a, hipEventRecord(V.e0, a->stream));
    hipLaunchKernelGGL(variants_count_kernel, dim3(blocks), dim3(256), 0, a->stream, d_rows, pitch, n, a->d_ref, a->plen, V.qc);
    HIPCHK(a, hipGetLastError());
    hipLaunchKernelGGL(variants_offsets_kernel, dim3(1), dim3(1024), 0, a->stream, V.qc, n, V.off);
    HIPCHK(a, hipGetLastError());
    HIPCHK(a, hipEventRecord(V.e1, a->stream));
    HIPCHK(a, hipMemcpyAsync(&total, V.off.p + n, sizeof total, hipMemcpyDeviceToHost, a->stream));
    HIPCHK(a, hipStreamSynchronize(a->stream));
    if (total < 0 || total > (long long)n * ((long long)a->plen + 1)) return afail(a, UVAIA_ALIGN_ESTATE, "%lld variant records for %d rows of %d sites", total, n, a->plen);
    if (total) {
      if ((rc = V.rec.reserve(a, (size_t)total))) return rc;
      HIPCHK(a, hipEventRecord(V.e2, a->stream));
      hipLaunchKernelGGL(variants_emit_kernel, dim3(blocks), dim3(256), 0, a->stream, d_rows, pitch, n, a->d_ref, a->plen, V.off, V.rec);
      HIPCHK(a, hipGetLastError());
      HIPCHK(a, hipEventRecord(V.e3, a->stream));
      HIPCHK(a, hipEventSynchronize(V.e3));
      HIPCHK(a, hipEventElapsedTime(&ms_emit, V.e2, V.e3));
    }
    HIPCHK(a, hipEventElapsedTime(&ms, V.e0, V.e1));
    V.ms += (double)ms + ms_emit;
    V.total = total;
  }
  V.n_rows = n; V.done = true;
  return 0;
}

struct CloseAligner { void operator()(uvaia_aligner *a) const { uvaia_align_close(a); } };

}  // namespace

extern "C" {

void uvaia_align_default_options(uvaia_align_options *opt)
{ // src/align.c:305-309
  if (!opt) return;
  opt->mismatch = 4; opt->gap_opening = 6; opt->gap_extension = 2;
  opt->min_wavefront_length = 128; opt->max_distance_threshold = 512;
  opt->workspace_bytes = 0; opt->max_blocks = 0;
}

const char *uvaia_align_last_error(const uvaia_aligner *a) { return a ? a->err.c_str() : g_align_open_error.c_str(); }

void uvaia_align_close(uvaia_aligner *a)
{
  if (!a) return;
  hipSetDevice(a->device);
  if (a->stream) hipStreamSynchronize(a->stream);
  delete a;
}

int uvaia_align_open(uvaia_aligner **out, const char *ref, int ref_len, int device, const uvaia_align_options *opt_in)
{
  if (!out) return UVAIA_ALIGN_EINVAL;
  *out = nullptr;
  if (!ref || ref_len < 1) return afail(nullptr, UVAIA_ALIGN_EINVAL, "empty reference sequence");
  uvaia_align_options opt; uvaia_align_default_options(&opt);
  if (opt_in) opt = *opt_in;
  if (opt.mismatch < 1 || opt.gap_opening < 0 || opt.gap_extension < 1 || opt.mismatch >= RING || opt.gap_opening + opt.gap_extension >= RING)
    return afail(nullptr, UVAIA_ALIGN_EINVAL, "mismatch and gap extension must be positive, gap opening not negative, mismatch and opening + extension below %d (mismatch %d, gap opening %d, gap extension %d)", RING, opt.mismatch, opt.gap_opening, opt.gap_extension);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return afail(nullptr, UVAIA_ALIGN_ENODEV, "no HIP device: the aligner runs on an MI355X (gfx950) and has no CPU path");
  if (device < 0 || device >= ndev) return afail(nullptr, UVAIA_ALIGN_EINVAL, "device %d out of range (%d devices)", device, ndev);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return afail(nullptr, UVAIA_ALIGN_ENODEV, "cannot query device %d", device);
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return afail(nullptr, UVAIA_ALIGN_ENODEV, "device %d is %s: this library is built for gfx950 only", device, prop.gcnArchName);
  int caller_device = -1;
  if (hipGetDevice(&caller_device) != hipSuccess) caller_device = -1;
  if (hipSetDevice(device) != hipSuccess) return afail(nullptr, UVAIA_ALIGN_ENODEV, "cannot select device %d", device);
  struct RestoreDevice { int d; ~RestoreDevice() { if (d >= 0) hipSetDevice(d); } } restore_{caller_device};   // every later call selects a->device itself
  std::unique_ptr<uvaia_aligner, CloseAligner> a(new uvaia_aligner());   // a failure below closes the half-made aligner; its message goes to uvaia_align_last_error(NULL)
  a->device = device; a->plen = ref_len;
  a->P.x = opt.mismatch; a->P.oe = opt.gap_opening + opt.gap_extension; a->P.e = opt.gap_extension;
  a->P.min_wf_len = opt.min_wavefront_length; a->P.max_dist_thr = opt.max_distance_threshold;
  { int g = a->P.x, b = a->P.oe; while (b) { const int t = g % b; g = b; b = t; } b = a->P.e; while (b) { const int t = g % b; g = b; b = t; } a->P.g = g; }
  // table size of affine_wavefronts_new_reduced (L, 3 L, ..): min(L, 3L) * mismatch + gap_opening + |L - 3L| * gap_extension
  const long long ms = (long long)ref_len * opt.mismatch + opt.gap_opening + 2LL * ref_len * opt.gap_extension;
  a->P.max_score = (int)std::min<long long>(ms, 0x3fffffff);
  a->workspace_request = opt.workspace_bytes;
  {   // as many blocks as the chip holds at once (the blocks are persistent: more would only queue behind them)
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, wfa_align_kernel, TPB, 0) != hipSuccess || per_cu < 1) per_cu = 4;
    a->max_blocks = opt.max_blocks > 0 ? opt.max_blocks : prop.multiProcessorCount * per_cu;
  }
  int rc;
  HIPCHK(nullptr, hipStreamCreateWithFlags(&a->stream.s, hipStreamNonBlocking));
  if ((rc = a->ev_a.make(nullptr)) || (rc = a->ev_b.make(nullptr)) || (rc = a->d_ref.reserve(nullptr, (size_t)ref_len + 512))) return rc;
  HIPCHK(nullptr, hipMemcpy(a->d_ref, ref, (size_t)ref_len, hipMemcpyHostToDevice));
  if ((rc = a->d_next.reserve(nullptr, 1)) || (rc = a->d_cells.reserve(nullptr, 1))) return rc;
  *out = a.release();
  return 0;
}

// A pool of n >= 1 queries whose bytes lie at bytes + offsets[0], in host memory or (kind = hipMemcpyDeviceToDevice) in the memory of the
// aligner's device: one copy into d_seqs, the offsets, and the order the queries are started in.  Returns when all of it is done.
static int load_pool(uvaia_aligner *a, const char *bytes, const int64_t *offsets, int n, hipMemcpyKind kind)
{
  const size_t total = (size_t)(offsets[n] - offsets[0]);
  int rc = ensure_pool(a, total, n); if (rc) return rc;
  a->h_off.resize((size_t)n + 1);
  for (int i = 0; i <= n; i++) a->h_off[(size_t)i] = (long long)(offsets[i] - offsets[0]);
  HIPCHK(a, hipStreamSynchronize(a->stream));
  if (total) HIPCHK(a, hipMemcpyAsync(a->d_seqs, bytes + offsets[0], total, kind, a->stream));
  HIPCHK(a, hipMemcpyAsync(a->d_off, a->h_off.data(), ((size_t)n + 1) * sizeof(long long), hipMemcpyHostToDevice, a->stream));
  {   // the order the queries are started in (d_status is free until the run: it takes the estimates)
    hipLaunchKernelGGL(expected_cost_kernel, dim3((unsigned)n), dim3(256), 0, a->stream, a->d_seqs, a->d_off, a->plen, n, a->d_status);
    HIPCHK(a, hipGetLastError());
    std::vector<int> cost((size_t)n), order((size_t)n);
    HIPCHK(a, hipMemcpyAsync(cost.data(), a->d_status, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, a->stream));
    HIPCHK(a, hipStreamSynchronize(a->stream));
    for (int i = 0; i < n; i++) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return cost[(size_t)x] > cost[(size_t)y]; });
    // a pool of fewer than three rounds of blocks stays in descending order throughout (longest first: with so few queries per block
    // the order is most of the launch's length, and the dearest third of such a pool in flight at once is what the workspace of the
    // library's choosing holds: measured at 2 000 queries); a larger one would put only its very dearest in flight at once
    if (a->workspace_request != 0 || (long long)n * 4 > (long long)a->max_blocks * 11) std::sort(order.begin(), order.begin() + n / 2);
    HIPCHK(a, hipMemcpyAsync(a->d_order, order.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, a->stream));
  }
  HIPCHK(a, hipStreamSynchronize(a->stream));
  a->n = n;
  return 0;
}

// what load_block and load_device refuse alike; 1 = an empty pool, nothing more to do
static int load_begin(uvaia_aligner *a, const void *bytes, const int64_t *offsets, int n)
{
  if (n < 0 || (n > 0 && (!bytes || !offsets))) return afail(a, UVAIA_ALIGN_EINVAL, "bad pool");
  HIPCHK(a, hipSetDevice(a->device));
  a->n = 0; a->ran = false; a->ins.done = false;
  if (a->var.from_run) a->var.done = false;
  if (n == 0) return 1;
  for (int i = 0; i < n; i++) if (offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[i] > 0x3fffffff) return afail(a, UVAIA_ALIGN_EINVAL, "bad length of sequence %d", i);
  return 0;
}

int uvaia_align_load_block(uvaia_aligner *a, const char *bytes, const int64_t *offsets, int n)
{
  if (!a) return UVAIA_ALIGN_EINVAL;
  if (int rc = load_begin(a, bytes, offsets, n)) return rc > 0 ? 0 : rc;
  return load_pool(a, bytes, offsets, n, hipMemcpyHostToDevice);
}

int uvaia_align_load_device(uvaia_aligner *a, const void *d_bytes, const int64_t *offsets, int n)
{
  if (!a) return UVAIA_ALIGN_EINVAL;
  if (int rc = load_begin(a, d_bytes, offsets, n)) return rc > 0 ? 0 : rc;
  // the bytes must be device memory of the aligner's device (asked of the runtime: the pointer is not dereferenced before) and
  // [offsets[0], offsets[n]) must lie inside its allocation
  if (offsets[0] < 0) return afail(a, UVAIA_ALIGN_EINVAL, "offsets[0] = %lld is negative", (long long)offsets[0]);
  hipPointerAttribute_t at;
  memset(&at, 0, sizeof at);
  if (hipPointerGetAttributes(&at, d_bytes) != hipSuccess) { (void)hipGetLastError(); return afail(a, UVAIA_ALIGN_EINVAL, "the sequences are not in device memory"); }
  if (at.type != hipMemoryTypeDevice || at.device != a->device)
    return afail(a, UVAIA_ALIGN_EINVAL, "the sequences must be in the memory of device %d (memory type %d, device %d)", a->device, (int)at.type, at.device);
  hipDeviceptr_t base = nullptr; size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, const_cast<void *>(d_bytes)) != hipSuccess) { (void)hipGetLastError(); return afail(a, UVAIA_ALIGN_EINVAL, "the sequences are not inside a device allocation"); }
  const size_t off = (size_t)(reinterpret_cast<const char *>(d_bytes) - reinterpret_cast<const char *>(base));
  if (off > size || (size_t)offsets[n] > size - off)
    return afail(a, UVAIA_ALIGN_EINVAL, "the sequences end beyond the device allocation they lie in (%lld bytes, %zu from its start, %zu in all)", (long long)offsets[n], off, size);
  return load_pool(a, static_cast<const char *>(d_bytes), offsets, n, hipMemcpyDeviceToDevice);
}

int uvaia_align_load(uvaia_aligner *a, const char *const *seq, const int *seq_len, int n)
{
  if (!a) return UVAIA_ALIGN_EINVAL;
  if (n < 0 || (n > 0 && (!seq || !seq_len))) return afail(a, UVAIA_ALIGN_EINVAL, "bad pool");
  std::vector<int64_t> off((size_t)n + 1, 0);
  for (int i = 0; i < n; i++) { if (seq_len[i] < 0 || !seq[i]) return afail(a, UVAIA_ALIGN_EINVAL, "bad sequence %d", i); off[(size_t)i + 1] = off[(size_t)i] + seq_len[i]; }
  a->h_bytes.resize((size_t)off[(size_t)n] + 1);
  for (int i = 0; i < n; i++) memcpy(a->h_bytes.data() + off[(size_t)i], seq[i], (size_t)seq_len[i]);
  return uvaia_align_load_block(a, a->h_bytes.data(), off.data(), n);
}

int uvaia_align_run(uvaia_aligner *a)
{
  if (!a) return UVAIA_ALIGN_EINVAL;
  HIPCHK(a, hipSetDevice(a->device));
  a->passes = 0; a->cells = 0; a->kernel_ms = 0; a->ran = false; a->ins.done = false;
  if (a->var.from_run || a->var.on) a->var.done = false;               // (with the option off, an answer of uvaia_align_variants_of stands)
  if (a->n == 0) {
    a->ins.h_rec.clear(); a->ins.h_bases.clear(); a->ins.done = a->ins.on;
    if (a->var.on) { if (int rc = run_variants(a, nullptr, 0, 0, true)) return rc; }
    a->ran = true;
    return 0;
  }
  int rc = ensure_pool_memory(a, false, nullptr); if (rc) return rc;
  HIPCHK(a, hipMemsetAsync(a->d_cells, 0, sizeof(unsigned long long), a->stream));
  HIPCHK(a, hipEventRecord(a->ev_a, a->stream));
  rc = run_passes(a); if (rc) return rc;
  if (a->ins.on) { rc = gather_insertions(a); if (rc) return rc; }
  HIPCHK(a, hipEventRecord(a->ev_b, a->stream));
  HIPCHK(a, hipEventSynchronize(a->ev_b));
  float ms = 0; HIPCHK(a, hipEventElapsedTime(&ms, a->ev_a, a->ev_b)); a->kernel_ms = ms;
  HIPCHK(a, hipMemcpy(&a->cells, a->d_cells, sizeof(unsigned long long), hipMemcpyDeviceToHost));
  if (a->var.on) { rc = run_variants(a, a->d_aln, (size_t)a->plen + 1, a->n, true); if (rc) return rc; }   // (after kernel_ms: the passes have a clock of their own)
  a->ran = true; a->ins.done = a->ins.on;
  return 0;
}

int uvaia_align_sync(uvaia_aligner *a)
{
  if (!a) return UVAIA_ALIGN_EINVAL;
  HIPCHK(a, hipSetDevice(a->device));
  HIPCHK(a, hipStreamSynchronize(a->stream));
  return 0;
}

int uvaia_align_fetch(uvaia_aligner *a, char *aln, int *score)
{
  if (!a) return UVAIA_ALIGN_EINVAL;
  if (!a->ran) return afail(a, UVAIA_ALIGN_ESTATE, "fetch without a completed run");
  if (a->n == 0) return 0;
  if (!aln && !score) return afail(a, UVAIA_ALIGN_EINVAL, "NULL row buffer");
  HIPCHK(a, hipSetDevice(a->device));
  if (aln) HIPCHK(a, hipMemcpyAsync(aln, a->d_aln, (size_t)a->n * ((size_t)a->plen + 1), hipMemcpyDeviceToHost, a->stream));   // (scores alone: the rows stay where they are)
  if (score) HIPCHK(a, hipMemcpyAsync(score, a->d_score, (size_t)a->n * sizeof(int), hipMemcpyDeviceToHost, a->stream));
  HIPCHK(a, hipStreamSynchronize(a->stream));
  return 0;
}

int uvaia_align_device_rows(uvaia_aligner *a, const void **d_rows, size_t *pitch, int *n, int *device)
{
  if (!a) return UVAIA_ALIGN_EINVAL;
  if (!a->ran) return afail(a, UVAIA_ALIGN_ESTATE, "no completed run whose rows could be handed out");
  if (d_rows) *d_rows = a->n ? a->d_aln.p : nullptr;
  if (pitch) *pitch = (size_t)a->plen + 1;
  if (n) *n = a->n;
  if (device) *device = a->device;
  return 0;
}

int uvaia_align_batch(uvaia_aligner *a, const char *const *seq, const int *seq_len, int n, char *aln, int *score)
{
  int rc = uvaia_align_load(a, seq, seq_len, n); if (rc) return rc;
  rc = uvaia_align_run(a); if (rc) return rc;
  return uvaia_align_fetch(a, aln, score);
}

int uvaia_align_set_insertions(uvaia_aligner *a, int on, size_t capacity_records)
{ // src/align.c:366-390 drops the characters of an I operation: with the option on the next runs keep where they were
  if (!a) return UVAIA_ALIGN_EINVAL;
  if (capacity_records > 0x7fffffff) return afail(a, UVAIA_ALIGN_EINVAL, "a record buffer of %zu records is more than a launch can address", capacity_records);
  a->ins.on = on != 0; a->ins.cap_request = capacity_records; a->ins.done = false;
  return 0;
}

int uvaia_align_insertion_counts(uvaia_aligner *a, long long *n_records, long long *n_bases)
{
  if (!a) return UVAIA_ALIGN_EINVAL;
  if (!a->ins.on || !a->ran || !a->ins.done) return afail(a, UVAIA_ALIGN_ESTATE, "%s", a->ins.on ?"no completed run that kept its insertions" : "insertions are not kept: uvaia_align_set_insertions was not called");
  if (n_records) *n_records = (long long)a->ins.h_rec.size();
  if (n_bases) *n_bases = (long long)a->ins.h_bases.size();
  return 0;
}

int uvaia_align_fetch_insertions(uvaia_aligner *a, uvaia_align_insertion *rec, char *bases)
{
  if (int rc = uvaia_align_insertion_counts(a, nullptr, nullptr)) return rc;
  if (rec && !a->ins.h_rec.empty()) memcpy(rec, a->ins.h_rec.data(), a->ins.h_rec.size() * sizeof(uvaia_align_insertion));
  if (bases && !a->ins.h_bases.empty()) memcpy(bases, a->ins.h_bases.data(), a->ins.h_bases.size());
  return 0;
}

int uvaia_align_set_variants(uvaia_aligner *a, int on)
{ // src/align.c:366-390 writes the rows: with the option on the next runs also say what each of them differs from the reference by
  if (!a) return UVAIA_ALIGN_EINVAL;
  a->var.on = on != 0;
  if (a->var.from_run) a->var.done = false;
  return 0;
}

int uvaia_align_variant_counts(uvaia_aligner *a, long long *n_records, int *n_rows)
{
  if (!a) return UVAIA_ALIGN_EINVAL;
  if (!a->var.done) return afail(a, UVAIA_ALIGN_ESTATE, "no variants yet: neither a completed run with uvaia_align_set_variants on nor uvaia_align_variants_of");
  if (n_records) *n_records = a->var.total;
  if (n_rows) *n_rows = a->var.n_rows;
  return 0;
}

int uvaia_align_fetch_variants(uvaia_aligner *a, uvaia_align_variant *rec, uvaia_align_row_qc *qc)
{
  if (int rc = uvaia_align_variant_counts(a, nullptr, nullptr)) return rc;
  HIPCHK(a, hipSetDevice(a->device));
  if (rec && a->var.total) HIPCHK(a, hipMemcpyAsync(rec, a->var.rec, (size_t)a->var.total * sizeof(uvaia_align_variant), hipMemcpyDeviceToHost, a->stream));
  if (qc && a->var.n_rows) HIPCHK(a, hipMemcpyAsync(qc, a->var.qc, (size_t)a->var.n_rows * sizeof(uvaia_align_row_qc), hipMemcpyDeviceToHost, a->stream));
  HIPCHK(a, hipStreamSynchronize(a->stream));
  return 0;
}

int uvaia_align_variants_of(uvaia_aligner *a, const char *rows, size_t pitch, int n)
{ // rows on the reference's columns that another aligner made, in place of those src/align.c:366-390 writes
  if (!a) return UVAIA_ALIGN_EINVAL;
  if (n < 0 || (n > 0 && !rows)) return afail(a, UVAIA_ALIGN_EINVAL, "bad rows (%d of them%s)", n, rows ? "" : ", NULL");
  if (pitch < (size_t)a->plen) return afail(a, UVAIA_ALIGN_EINVAL, "pitch %zu is below the %d sites of a row", pitch, a->plen);
  HIPCHK(a, hipSetDevice(a->device));
  if (n == 0) return run_variants(a, nullptr, pitch, 0, false);
  const size_t bytes = (size_t)(n - 1) * pitch + (size_t)a->plen;      // (the last row may end with its last site)
  a->var.done = false;
  HIPCHK(a, hipStreamSynchronize(a->stream));
  if (int rc = a->var.rows.reserve(a, bytes + 16)) return rc;          // (the load of 16 sites reads whole dwords)
  HIPCHK(a, hipMemcpyAsync(a->var.rows, rows, bytes, hipMemcpyHostToDevice, a->stream));
  return run_variants(a, a->var.rows, pitch, n, false);
}

double uvaia_align_variants_ms(uvaia_aligner *a, int reset)
{
  if (!a) return 0.;
  const double ms = a->var.ms;
  if (reset) a->var.ms = 0;
  return ms;
}

int uvaia_align_stats(uvaia_aligner *a, unsigned long long *cells, double *wavefront_bytes, int *passes, double *kernel_ms)
{
  if (!a) return UVAIA_ALIGN_EINVAL;
  if (cells) *cells = a->cells;
  if (wavefront_bytes) *wavefront_bytes = (double)a->cells * 33.0;     // per cell: M offset + provenance byte kept, I and D offsets to the ring, five offsets read
  if (passes) *passes = a->passes;
  if (kernel_ms) *kernel_ms = a->kernel_ms;
  return 0;
}

}  // extern "C"
