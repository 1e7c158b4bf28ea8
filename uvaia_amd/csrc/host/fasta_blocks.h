/*
 * fasta_blocks.h -- FASTA text read in blocks for a parser that takes whole blocks (`uvaiapack --device-parse`: uvaia_gpu_fasta_scan,
 * include/uvaia_gpu.h), and fasta_scan_host, the plain C restatement of that parser's first pass.  Own code, no counterpart in the reference.
 *
 * The block reader: two buffers of block_bytes (64 MiB by default -- a design choice: some two thousand genomes of 30 000 sites per scan, so
 * that launches and copies back are amortised, and 128 MiB of page-locked memory in all).  A reader thread fills one from the file or the
 * decompressor's pipe while the records of the other are packed; the tail a scan did not consume (the record its block cuts) is copied to
 * the front of the next buffer before that is filled, so every block begins at a header line.  The scan step is a callback: the device
 * parser in the command, fasta_scan_host in the CPU tests and in tools/fasta_blocks_check.c.
 */
#ifndef UVAIA_HOST_FASTA_BLOCKS_H
#define UVAIA_HOST_FASTA_BLOCKS_H

#include <stddef.h>
#include <stdint.h>

#include "../../../include/uvaia_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FASTA_BLOCK_BYTES ((size_t) 64 << 20)

enum { FASTA_BAD_NONE = 0, FASTA_BAD_NUL = 1, FASTA_BAD_TEXT = 2, FASTA_BAD_EMPTY = 3 };

/* Pass 1 of kernels_fasta.inc in plain C, with the contract of uvaia_gpu_fasta_scan: rec[0 .. max_records) takes the complete records of
 * text[0 .. n), *consumed is where the header line of the first record not returned begins.  Returns 0, or -1 on irregular input among
 * what would be returned, with its kind (FASTA_BAD_*) and byte offset: the text before the first header line first, then the records in
 * their order, a NUL before a missing sequence. */
int fasta_scan_host (const char *text, size_t n, int final, int max_records, uvaia_gpu_fasta_record *rec, int *n_records, size_t *consumed, int *bad_kind, size_t *bad_off);
/* the cleaned sequence of a record (white space dropped, a-z upper-cased) into out[0 .. rec->seq_len); returns the bytes written */
size_t fasta_clean_host (const char *text, const uvaia_gpu_fasta_record *rec, char *out);
/* the body bytes of a record that are one of A C G T a c g t: uvaia_gpu_fasta_acgt in plain C, the first counter of
 * biomcmc_count_sequence_acgt on the cleaned sequence (the second is seq_len - non_n of the record) */
int fasta_count_acgt_host (const char *text, const uvaia_gpu_fasta_record *rec);

/* the scan step: 0 with *n_records and *consumed; or -1, for irregular text with its kind (FASTA_BAD_*) and its offset within text, for
 * anything else with *bad_kind left FASTA_BAD_NONE and a message */
typedef int (*fasta_scan_fn) (void *user, const char *text, size_t n, int final, int *n_records, size_t *consumed, int *bad_kind, size_t *bad_off, char *err, size_t errlen);
/* what becomes of the records of one scan: called after every scan that returned some, before the text is scanned further.  It may write to
 * text[0 .. consumed) (the command ends the names there with a NUL).  0, or -1 with a message */
typedef int (*fasta_records_fn) (void *user, char *text, size_t consumed, int n_records, char *err, size_t errlen);

typedef struct fasta_blocks_struct *fasta_blocks;

/* alloc / release: where the two buffers come from (NULL, NULL: malloc and free); NULL with a message when the file or the memory is not to be had */
fasta_blocks fasta_blocks_open (const char *path, size_t block_bytes, void *(*alloc) (size_t), void (*release) (void *), char *err, size_t errlen);
/* Reads the whole stream: scan, hand the records over; a scan that returned max_records (its cap) is followed by one of what lies behind
 * them in the same block.  As soon as a block's tail is known -- after its last scan, before the records of that scan are handed over --
 * the reader thread fills the other buffer behind a copy of the tail.  0 at the end of the stream; -1 with a message that names the file
 * and the byte of the stream for irregular input, a record that does not fit a block (by its name) and what the callbacks refuse.
 * *n_bytes (may be NULL): bytes read. */
int fasta_blocks_run (fasta_blocks fb, int max_records, fasta_scan_fn scan, void *scan_user, fasta_records_fn records, void *records_user, uint64_t *n_bytes, char *err, size_t errlen);
/* after a run that read the stream to its end: closes it; -1 with a message when the decompressor failed mid-stream (what looked like the
 * end of the data was not), 0 otherwise */
int fasta_blocks_finish (fasta_blocks fb, char *err, size_t errlen);
/* gives up a stream that was not read to its end */
void fasta_blocks_close (fasta_blocks fb);

/* fasta_scan_host as a scan step (user: a struct fasta_host_scan, whose table the step fills), and the whole of a file through the block reader and fasta_scan_host written as
 * ">name\nSEQUENCE\n" per record to out_path: what the CPU tests compare with readfasta_next */
struct fasta_host_scan { int max_records, n_records; uvaia_gpu_fasta_record *rec; };     /* rec: room for max_records entries */
int fasta_scan_host_step (void *user, const char *text, size_t n, int final, int *n_records, size_t *consumed, int *bad_kind, size_t *bad_off, char *err, size_t errlen);
int fasta_blocks_normalise_host (const char *path, size_t block_bytes, int max_records, const char *out_path, char *err, size_t errlen);

#ifdef __cplusplus
}
#endif
#endif
