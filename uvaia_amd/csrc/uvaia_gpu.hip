// uvaia_gpu.hip -- MI355X (gfx950 / CDNA4) engine behind include/uvaia_gpu.h.
//
// What it replaces in the reference (paths under /root/reference): the three OpenMP loops of
// src/nearest.c:293-306 -- consensus pre-score, per-query gate + heap update, is_best OR -- and the scoring
// kernels they call (src/fastaseq.c:585-596 and the absent biomcmc 4-count kernel, see oracle/uvaia_oracle.h).
//
// Design:
//   * sequences live in HBM as bit-planes, interleaved per tile of 64 references so that one lane owns one
//     reference: tile[t][w4][plane][lane] is a uint4 holding alignment words 4*w4..4*w4+3 (32 sites per word) of
//     that plane for reference 64*t+lane.  One wave-wide dwordx4 load = 1 KiB contiguous.
//   * the scan kernel keeps QT queries' accumulators in VGPRs; query words are wave-uniform and arrive through
//     scalar loads (SGPR operands of v_bitop3/v_and/v_xor), so the inner loop is pure VALU + v_bcnt with no
//     LDS traffic and no cross-lane reduction.  No MFMA: this is a popcount scan.
//   * the order-dependent gate/heap state machine of src/nearest.c:479-510 runs on the device, one wave per
//     query, over the dense pair counts of a batch, reproducing the reference's heap layout slot for slot.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <mutex>
#include <numeric>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "../../include/uvaia_gpu.h"
#include "iupac_decode.h"
#include "rows_block.h"

// ------------------------------------------------------------------------------------------------------------
// small helpers
// ------------------------------------------------------------------------------------------------------------
#define TT_A 0xF0u   // v_bitop3 truth-table columns: src0, src1, src2
#define TT_B 0xCCu
#define TT_C 0xAAu
#define B3(a, b, c, tt) __builtin_amdgcn_bitop3_b32((a), (b), (c), (tt) & 0xFFu)

static __device__ __forceinline__ uint32_t u4c(const uint4 &v, int j)
{ // component j of a uint4; folds to a register pick once j is a constant (no address is taken)
  return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w;
}

typedef uint32_t u32x4_ld __attribute__((ext_vector_type(4)));
static __device__ __forceinline__ uint4 ld_stream(const uint4 *p)
{ // packed planes a kernel reads exactly once: a non-temporal load (the packed-plane scans went from 0.69 to 0.77 of the HBM peak with it)
  const u32x4_ld v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_ld *>(p));
  return make_uint4(v.x, v.y, v.z, v.w);
}

static __device__ __forceinline__ int bcnt_acc(uint32_t x, int acc)
{ // v_bcnt_u32_b32 d, x, acc : popcount with free accumulate (keeps one VALU op per count and word)
  int r;
  asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
  return r;
}

namespace {

constexpr int HEAP_ENTRY = 8;          // 6 scores + 64-bit ordinal (lo, hi)
constexpr int AMB_CAP = 11;            // alignment words with a partially ambiguous site remembered per sequence
constexpr int AMB_STRIDE = AMB_CAP + 1;  // ints per QUERY: count (uncapped) + word indices
constexpr int AMB_ROW = 64;            // ints per REFERENCE side row (256 B, one coalesced wave load):
                                       //   [0] count (uncapped)  [1..11] word indices  [12 + 4k + p] plane p of the k-th listed word
constexpr int PACK_CHUNK = 4096;       // references per host->device staging round (multiple of 64)
constexpr uint32_t SCAN3_BIAS = 16384u; // scan3_kernel: bias of a pair's low counter half (what the rare items and, --acgt, the polymorphic columns may take away)
constexpr int NBUF = 4;                // counter buffers: the scan may run this many slices ahead of the gate/replay

}  // namespace

#include "kernels_pack.inc"
#include "kernels_rows.inc"
#include "kernels_consensus.inc"
#include "kernels_scan2.inc"
#include "kernels_scan3.inc"
#include "kernels_replay.inc"
#include "kernels_ball.inc"
#include "kernels_qprep.inc"
#include "kernels_expand.inc"
#include "kernels_encode.inc"
#include "kernels_fasta.inc"
#include "kernels_pairs.inc"

// ------------------------------------------------------------------------------------------------------------
// host side, in sections (one translation unit: the kernels above are templates the sections instantiate); the context and everything
// else the host owns is in host_ctx.inc, so that this file changes only with what the kernels themselves see
// ------------------------------------------------------------------------------------------------------------
#include "host_ctx.inc"
#include "host_launch.inc"
#include "host_qtables.inc"
#include "host_qprep.inc"
#include "host_open.inc"
#include "host_batch.inc"
#include "host_resident.inc"
#include "host_rows.inc"
#include "host_text.inc"
#include "host_shards.inc"
#include "host_ball.inc"
#include "host_window.inc"
#include "host_encode.inc"
#include "host_fasta.inc"
#include "host_pairs.inc"
