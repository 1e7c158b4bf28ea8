/*
 * uvdb.h -- packed on-disk reference database.  Own format, no counterpart in the reference: it replaces,
 * for a database that is searched more than once, the serial text path readfasta_next() (src/fastaseq.c:422-474) + the slot
 * filling loop of src/nearest.c:251-286 (length check, -A filter, quick_count_sequence_non_N) by arrays the GPU engine takes
 * as they are (uvaia_gpu_db_append_packed, include/uvaia_gpu.h).
 *
 * File (little endian, sections 64-byte aligned, offsets from the start of the file):
 *   header   struct uvdb_header
 *   planes   n_tiles x tile_bytes    tiles of 64 references, [word group][plane A,C,G,T][lane] 16-byte words
 *   non_n    n_tiles*64 x int32      valid sites of every reference (what the -A filter and score 6 use)
 *   side     n_tiles*64 x side_row_ints x int32   partially ambiguous words of every reference
 *   name_idx (n_ref+1) x uint64      byte offsets into names
 *   names    NUL-terminated names, in stream order
 *   exc_idx  (n_ref+1) x uint64      record offsets into exc
 *   exc      (uint32 pos, uint32 len<<8 | char)   runs of invalid sites whose character is not 'N' ('-', '?', 'X', 'O', '.'):
 *            with them the exact (upper-case) text of a reference is recovered from its planes, as the .aln.xz dump needs
 * References that fail the -A filter or the length check are not stored: the filter value is recorded in the header.
 *
 * Version 2, the compact form (`uvaiapack --compact`): a disk and transport format only.  Aligned genomes of one pathogen are nearly
 * identical column by column, so the file holds one base row and, per reference, the 32-site words in which it differs from the base.
 * Header, non_n, name_idx, names, exc_idx and exc keep their version 1 form; planes and side are replaced (the side rows are a pure
 * function of the planes and are not stored):
 *   base     W4*4 x 16 bytes         one reference's worth of planes, [word group][plane A,C,G,T] 16-byte words (header field off_planes).
 *            A plane bit is set exactly when it is set in more than half of the first min (n_ref, UVDB_BASE_SAMPLE) stored references;
 *            bits at and beyond nchar are zero.  Correctness never depends on the base: the rule makes files reproducible.
 *   non_n    n_tiles*64 x int32      as version 1
 *   head_idx (n_tiles*64+1) x uint64 record offsets into heads (header field off_side), one entry per LANE of the dense tiles
 *   heads    uint32 records (header field reserved[0]): first_word:16 | n_words:11 | literal:1 | code:4, most significant first.  Word w of
 *            a reference covers sites 32w .. 32w+31; n_words is 1 .. 2047.  A fill head (literal = 0) says every site of those words has the
 *            4-bit set `code`: plane p of each word is all ones if bit p of code is set, zero otherwise (code 0: an N or gap run).  A
 *            literal head says the next n_words x 4 dwords of lits are planes A, C, G, T of each of those words.
 *   lit_idx  (n_tiles*64+1) x uint64 offsets into lits, in words of 16 bytes (header field reserved[1])
 *   lits     16 bytes per literal word, starts at the next multiple of 64 behind lit_idx
 * The two index sections cover the lanes of whole tiles, not n_ref + 1 entries: the lanes past the last reference are all-zero rows
 * encoded against the base like any other, so that a staged range of whole tiles (uvaia_gpu_db_stage_compact_at, include/uvaia_gpu.h)
 * expands to the zero lanes a dense file holds without knowing where the file ends.
 * Canonical encoding: a word equal to the base's word has no record; a differing word whose four planes are each 0 or 0xFFFFFFFF is a
 * fill, any other a literal; adjacent words of the same kind (fills: and the same code) are one head, cut only at 2047 words; heads
 * ascend and never overlap; the padding words beyond nchar never differ from the base.  first_word has 16 bits: a compact file is
 * refused for nchar > UVDB_COMPACT_MAX_NCHAR.  uvdb_open checks every index and every head of a version 2 file (OpenMP: it is a pass
 * over the whole file), so the device never sees an unchecked head.
 * Several files are read as one stream through uvdb_set.h (a repeated --packed); `uvaiapack --merge` joins files into the one file their
 * texts would have been packed to, and is where a recorded -A is tightened (a filter cannot be loosened: the rows are not there).
 */
#ifndef UVAIA_HOST_UVDB_H
#define UVAIA_HOST_UVDB_H

#include <stdint.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UVDB_MAGIC "UVAIADB1"
#define UVDB_SIDE_ROW_INTS 64   /* ints per side row: [0] count, [1..11] listed alignment words, [12 + 4k + p] plane p of the k-th listed word (uvaia_gpu_db_side_row_ints()) */
#define UVDB_SIDE_LISTED 11

struct uvdb_header {
  char magic[8];
  uint32_t version, nchar, W4, side_row_ints;
  uint64_t n_ref, n_tiles, tile_bytes;
  double ref_ambiguity;                 /* -A used while packing */
  uint64_t off_planes, off_nonn, off_side, off_name_idx, off_names, off_exc_idx, off_exc, file_bytes;
  uint64_t reserved[2];
};

typedef struct { uint32_t pos, len_char; } uvdb_exc;

#define UVDB_BASE_SAMPLE 4096            /* references the base row of a version 2 file is the majority of */
#define UVDB_COMPACT_MAX_NCHAR 2097152   /* 65 536 words of 32 sites: what first_word counts */
#define UVDB_HEAD_MAX_WORDS 2047
#define UVDB_HEAD(first, n, lit, code) (((uint32_t) (first) << 16) | ((uint32_t) (n) << 5) | ((uint32_t) (lit) << 4) | (uint32_t) (code))
#define UVDB_HEAD_FIRST(h)   ((uint32_t) (h) >> 16)
#define UVDB_HEAD_WORDS(h)   (((uint32_t) (h) >> 5) & 0x7FFu)
#define UVDB_HEAD_LITERAL(h) (((uint32_t) (h) >> 4) & 1u)
#define UVDB_HEAD_CODE(h)    ((uint32_t) (h) & 15u)

/* ---- writer: tiles are appended in stream order, the index sections go to the end on close */
typedef struct uvdb_writer_struct *uvdb_writer;
uvdb_writer uvdb_create (const char *filename, int nchar, size_t tile_bytes, int side_row_ints, double ref_ambiguity);
/* text of the next reference: recorded for the name table and the exception runs (the planes come from the engine) */
int uvdb_add_reference (uvdb_writer w, const char *name, const char *seq);
/* the same for a reference whose text is not on the host: its exception runs as records (pos, len << 8 | char), by position, as the rule
 * above gives them (a maximal stretch of one of - ? X O . , cut at 0xFFFFFF sites); uvdb_add_reference computes them from the text and
 * calls this.  The engine computes them from rows in device memory (uvaia_gpu_rows_census + uvaia_gpu_rows_exceptions). */
int uvdb_add_reference_runs (uvdb_writer w, const char *name, const uvdb_exc *runs, size_t n_runs);
/* the next n_tiles tiles in the engine's export form */
int uvdb_add_tiles (uvdb_writer w, size_t n_tiles, const void *planes, const int *non_n, const int *side_rows);
int uvdb_close (uvdb_writer w);       /* 0 on success */
/* a version 2 file: the same calls follow.  The writer ignores side rows (NULL will do); it keeps the tiles until it has UVDB_BASE_SAMPLE
 * references or is closed, then fixes the base and encodes that chunk on the host; later ones it encodes on the host as well
 * (uvdb_add_tiles) or takes as records (uvdb_add_tiles_encoded).  NULL also for nchar > UVDB_COMPACT_MAX_NCHAR. */
uvdb_writer uvdb_create_compact (const char *filename, int nchar, size_t tile_bytes, int side_row_ints, double ref_ambiguity);
/* the base of a version 2 writer, [word group][plane A,C,G,T] 16-byte words, once it is fixed (the rule above: from the pending dense tiles, when
 * the sample is complete); NULL before that and for a version 1 writer */
const uint32_t *uvdb_compact_base (uvdb_writer w);
/* the next n_tiles tiles of a version 2 writer whose base is fixed, as records somebody else encoded against that base (the engine:
 * uvaia_gpu_db_encode_compact + uvaia_gpu_db_encoded_records, include/uvaia_gpu.h): non_n n_tiles * 64 counts; head_idx / lit_idx
 * n_tiles * 64 + 1 offsets each, from any start -- they are rebased onto the file's running totals; heads / lits: the arrays the offsets
 * count from (lits in words of 16 bytes).  The records are checked as uvdb_open checks a file's -- no empty head, none leaving the
 * alignment, ascending without overlap, the literal heads of a lane adding up to its extent of lits -- and -1 is returned with nothing
 * appended instead of writing a file uvdb_open would refuse.  -1 also before the base is fixed and for a version 1 writer. */
int uvdb_add_tiles_encoded (uvdb_writer w, size_t n_tiles, const int *non_n, const uint64_t *head_idx, const uint32_t *heads, const uint64_t *lit_idx, const uint32_t *lits);

/* ---- reader: the file is mapped read-only; every pointer below points into the mapping */
typedef struct uvdb_reader_struct {
  struct uvdb_header h;
  const unsigned char *map; size_t map_len;
  const uint64_t *name_idx; const char *names;
  const uint64_t *exc_idx; const uvdb_exc *exc;
  const int32_t *non_n;
  /* version 2 only (NULL otherwise) */
  const uint32_t *base; const uint64_t *head_idx; const uint32_t *heads; const uint64_t *lit_idx; const uint32_t *lits;
} *uvdb_reader;
uvdb_reader uvdb_open (const char *filename, char *errbuf, size_t errlen);
const char *uvdb_name (uvdb_reader r, uint64_t i);
/* version of the file's header without opening it (0: not a packed database or unreadable): for refusals before any other work */
uint32_t uvdb_file_version (const char *filename);
/* both NULL for a version 2 reader, which holds no dense tiles: every caller handles that or refuses the file earlier */
const void *uvdb_tile_planes (uvdb_reader r, uint64_t tile);        /* h.tile_bytes per tile, consecutive tiles are contiguous */
const int32_t *uvdb_tile_side_rows (uvdb_reader r, uint64_t tile);   /* 64 * h.side_row_ints ints per tile, contiguous */
/* Tiles first_tile .. first_tile + n_tiles - 1 as dense tiles, expanded on the CPU (a version 1 reader: copied): planes_out n_tiles x
 * h.tile_bytes; side_rows_out (may be NULL) n_tiles x 64 x h.side_row_ints ints in the fixed form of the engine's side_rows_canonical_kernel
 * -- the partially ambiguous words in ascending order, the first UVDB_SIDE_LISTED listed with their planes, [0] their total.  Lanes
 * past n_ref come out as zeros.  0 on success. */
int uvdb_expand_tiles (uvdb_reader r, uint64_t first_tile, uint64_t n_tiles, void *planes_out, int32_t *side_rows_out);
/* exact upper-case text of reference i (nchar + 1 bytes) */
void uvdb_unpack_reference (uvdb_reader r, uint64_t i, char *out);
/* the second half of it: the exception runs of reference i written over a row of nchar characters decoded from its planes elsewhere
 * (uvaia_gpu_unpack_rows, include/uvaia_gpu.h) */
void uvdb_apply_exceptions (uvdb_reader r, uint64_t i, char *row);
/* Can a file packed with -A pack_ambiguity answer a radius search run with -A ball_ambiguity exactly?  `uvaiaball` keeps a reference
 * with at least (int) (nchar * A) valid sites (src/ball.c:201), `uvaiapack` stored those with at least (int) (nchar * (1 - A_pack))
 * (src/nearest.c:263-268): the stored valid-site counts let the radius search apply its own filter, which sees every reference it
 * would have kept if and only if its threshold is not below the one of the file.  Both values as the command lines clamp them
 * (0.001 .. 1).  1 = exact, 0 = references may be missing. */
int uvdb_radius_filter_is_exact (int nchar, double ball_ambiguity, double pack_ambiguity);
void uvdb_close_reader (uvdb_reader r);

#ifdef __cplusplus
}
#endif
#endif
