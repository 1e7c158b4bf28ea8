// iupac_decode.h -- the one device helper that turns plane bits of the packed interchange form back into IUPAC characters.  Included by
// uvaia_gpu.hip (unpack_rows_kernel, kernels_pack.inc) and by uvaia_cluster.hip (clust_unpack_tiles_kernel).
#ifndef UVAIA_IUPAC_DECODE_H
#define UVAIA_IUPAC_DECODE_H

#include <hip/hip_runtime.h>

#include <cstdint>

// Per site the character is code[A | C << 1 | G << 2 | T << 3]; the empty set reads 'N' here, the sparse exception runs ('-', '?', 'X',
// 'O', '.') are the caller's.  Four sites at a time: the four bits of a plane are spread to the low bits of four bytes by one multiply, the
// sixteen-entry table is two v_perm_b32 (entries 0-7, 8-15) and a byte-wise select on bit 3.
static __device__ __forceinline__ uint32_t iupac_text4(uint32_t a, uint32_t c, uint32_t g, uint32_t t)
{ // a, c, g, t: four plane bits each (bit i = site i); returns the four characters, site 0 in the low byte
  constexpr uint32_t SPREAD = 0x00204081u, LOW = 0x01010101u;                    // bit i -> bit 8 i (the partial products do not overlap)
  const uint32_t set = ((a * SPREAD) & LOW) | (((c * SPREAD) & LOW) << 1) | (((g * SPREAD) & LOW) << 2) | (((t * SPREAD) & LOW) << 3);
  const uint32_t sel = set & 0x07070707u, high = ((set >> 3) & LOW) * 0xFFu;
  const uint32_t lo = __builtin_amdgcn_perm(0x56535247u /* G R S V */, 0x4D43414Eu /* N A C M */, sel);
  const uint32_t hi = __builtin_amdgcn_perm(0x4E42444Bu /* K D B N */, 0x48595754u /* T W Y H */, sel);
  return (lo & ~high) | (hi & high);
}

#endif
