/*
 * pack_main.c -- `uvaiapack`: aligned reference FASTA (raw/gz/xz/bz2, several files) -> packed database (uvdb.h).
 * No counterpart in the reference.  The filters of the reference's slot-filling loop that do not depend on
 * the queries are applied here once: the length check and the -A ambiguity filter (src/nearest.c:263-268).  The packing itself
 * runs on the GPU (uvaia_gpu_db_append + uvdb_export_tiles, uvdb_packer.h): the file holds exactly what the engine keeps resident.  Own code.
 *
 * `uvaiapack --merge`: packed databases -> one packed database, without their text: the file the same command without --merge writes from
 * the texts the inputs were packed from, byte for byte.  The tiles of an input are staged as the file holds them and its references
 * appended behind the resident ones on the device (uvaia_gpu_db_append_staged: an input rarely ends on a tile boundary); a tighter -A
 * drops rows through the selection of that call.
 *
 * `uvaiapack --compact` writes version 2 of the format (uvdb.h: a base row and per-reference differences, expanded on the GPU by
 * `uvaia --packed`), from texts or, with --merge, from packed inputs of either version; --merge without it reads both versions and
 * writes version 1, the way back to the dense file.  Once the base row is fixed (the first 4 096 references) the tiles are encoded on the
 * GPU and only their records cross the bus (uvdb_export_tiles).
 *
 * `uvaiapack --unpack` is the way back: the references of packed databases of either version as FASTA, decoded on the GPU out of the
 * staging slots (uvdb_extract.h), all of them or those a list of names asks for.  `uvaiapack --list` prints the stored names and needs no GPU.
 *
 * `uvaiapack --device-parse` (off by default) writes the same file from the same texts without the line reader: the decompressed bytes are
 * read in blocks (fasta_blocks.h), split into records and rows on the GPU (uvaia_gpu_fasta_scan, uvaia_gpu_fasta_rows) and packed from the
 * rows where they lie (uvdb_packer.h).  Only the names are taken from the host's copy of the text.
 */
#define _GNU_SOURCE
#include <getopt.h>
#include <libgen.h>

#include "cli_common.h"
#include "fastaseq.h"
#include "uvdb.h"
#include "uvdb_set.h"
#include "uvdb_packer.h"
#include "uvdb_extract.h"
#include "fasta_blocks.h"
#include "../../../include/uvaia_gpu.h"

#define PACK_BATCH 4096      /* references per engine round trip (a multiple of 64) */

static void
usage (const char *prog)
{
  printf ("%s \n", UVAIA_PACKAGE_STRING);
  printf ("Packs an aligned reference FASTA into the bit-plane database the MI355X engine searches without parsing text.\n\n");
  printf (" %s [-hv] [-A <double>] [--compact] [--device=<int>] -o <out.uvdb> <ref.fa(.gz,.xz)> [<ref.fa(.gz,.xz)>]...\n", prog);
  printf (" %s --device-parse [-A <double>] [--compact] [--device=<int>] -o <out.uvdb> <ref.fa(.gz,.xz)> [<ref.fa(.gz,.xz)>]...\n", prog);
  printf (" %s --merge [-A <double>] [--compact] [--device=<int>] -o <out.uvdb> <a.uvdb> [<b.uvdb>]...\n", prog);
  printf (" %s --unpack (-o <without suffix> | --stdout) [--names <file>] [--device=<int>] <a.uvdb> [<b.uvdb>]...\n", prog);
  printf (" %s --list <a.uvdb> [<b.uvdb>]...\n\n", prog);
  printf ("  -A, --ref_ambiguity=<double>     maximum allowed ambiguity for a REFERENCE sequence to be kept (default=0.5); `uvaia --packed` is run with the value of its file\n");
  printf ("  --device-parse                   split the text into sequences on the GPU instead of reading it line by line: the same file, from regular FASTA\n");
  printf ("                                   only (a NUL byte, text before the first header and a header without sequence are refused).  Not with --merge,\n");
  printf ("                                   --unpack or --list\n");
  printf ("  --merge                          the inputs are packed databases: joins them, in order, into the file that packing their texts together gives.\n");
  printf ("                                   -A then defaults to the inputs' common value; a smaller one drops the rows it excludes, a larger one than\n");
  printf ("                                   an input's is refused (that input no longer holds the rows it would keep)\n");
  printf ("  --compact                        write the compact form: one base row and, per reference, the 32-site words that differ from it; several times\n");
  printf ("                                   smaller for genomes of one pathogen.  `uvaia --packed` expands it on the GPU (one device); `uvaiaball` and\n");
  printf ("                                   `uvaiaclust` need the dense file, which `--merge -o dense.uvdb compact.uvdb` writes.  --merge reads both forms\n");
  printf ("  --unpack                         the inputs are packed databases (dense or compact, filtered with any -A): writes their references, in order, as\n");
  printf ("                                   FASTA -- the stored name, the upper-case text with - ? X O . where the input had them -- to <prefix>.aln.xz (-o)\n");
  printf ("                                   or uncompressed to standard output (--stdout); decoded on the GPU.  Not with --merge, --compact or -A\n");
  printf ("  --stdout                         with --unpack: uncompressed FASTA on standard output instead of -o\n");
  printf ("  --names=<file>                   with --unpack: only the references whose name is a line of <file>, every reference that carries such a name, in\n");
  printf ("                                   stream order; names that match nothing are listed on stderr\n");
  printf ("  --list                           prints the stored names of the packed databases given, one per line, in stream order (no GPU, no other option)\n");
  printf ("  -o, --output=<file>              packed database to write (--unpack: prefix of the xzipped alignment)\n");
  printf ("  --device=<int>                   GPU to use (default: current device)\n");
  printf ("Sequences that still have to be aligned: `uvaialign --packed <out.uvdb>` writes the same file straight from the aligner, without the text in between.\n");
}

/* the engine needs some query to exist: a plain ACGT string of the alignment's length */
static uvaia_gpu_ctx *
open_engine (int nchar, int device)
{
  uvaia_gpu_ctx *gpu = NULL;
  char *dummy = (char *) biomcmc_malloc ((size_t) nchar + 1);
  for (int s = 0; s < nchar; s++) dummy[s] = "ACGT"[s & 3];
  dummy[nchar] = '\0';
  const char *one[1] = {dummy};
  uvaia_gpu_query q;
  memset (&q, 0, sizeof q);
  q.n_query = 1; q.nchar = nchar; q.seq = one; q.consensus = dummy;
  if (uvaia_gpu_open (&gpu, &q, 1, device, PACK_BATCH)) biomcmc_error ("%s", uvaia_gpu_last_error (NULL));
  free (dummy);
  return gpu;
}

/* `uvaiapack --list` */
static int
list_main (int n_in, char **in)
{
  char msg[1024];
  if (n_in > UVDB_SET_MAX_FILES) biomcmc_error ("--list: at most %d packed databases", UVDB_SET_MAX_FILES);
  uvdb_set set = uvdb_set_open ((const char *const *) in, n_in, UVDB_SET_ANY_AMBIGUITY, msg, sizeof msg);
  if (!set) biomcmc_error ("%s", msg);
  for (uint64_t i = 0; i < set->n_ref; i++) printf ("%s\n", uvdb_set_name (set, i));
  uvdb_set_close (set);
  return EXIT_SUCCESS;
}

/* `uvaiapack --unpack` */
typedef struct { file_compress_t xz; int errors; } unpack_out;

static int
unpack_record (void *user, uint64_t k, uint64_t stream, const char *name, const char *row)
{
  unpack_out *u = (unpack_out *) user;
  if (u->xz) { write_fasta_record (u->xz, name, row); return 0; }
  if (printf (">%s\n%s\n", name, row) < 0) u->errors++;
  return u->errors;
}

static int
unpack_main (int n_in, char **in, const char *prefix, const char *names_file, int device)
{
  char msg[1024];
  int64_t time0[2];
  biomcmc_get_time (time0);
  if (n_in > UVDB_SET_MAX_FILES) biomcmc_error ("--unpack: at most %d packed databases", UVDB_SET_MAX_FILES);
  uvdb_name_list names = NULL;
  if (names_file && !(names = uvdb_name_list_read (names_file, msg, sizeof msg))) biomcmc_error ("%s", msg);
  uvdb_set set = uvdb_set_open ((const char *const *) in, n_in, UVDB_SET_ANY_AMBIGUITY, msg, sizeof msg);
  if (!set) biomcmc_error ("%s", msg);
  /* --names: every reference that carries a listed name, by position */
  uint64_t *pos = NULL, n = set->n_ref;
  if (names) {
    pos = (uint64_t *) biomcmc_malloc ((size_t) (set->n_ref ? set->n_ref : 1) * sizeof (uint64_t));
    n = 0;
    for (uint64_t i = 0; i < set->n_ref; i++) if (uvdb_name_list_find (names, uvdb_set_name (set, i)) >= 0) pos[n++] = i;
  }
  size_t outlength = 0;
  char *outfilename = prefix ? outfile_from_prefix (prefix, &outlength) : NULL;
  /* the engine and the tile layout first: a command that cannot run leaves no output file behind */
  uvaia_gpu_ctx *gpu = n ? open_engine ((int) set->nchar, device) : NULL;
  if (gpu && (set->side_row_ints != (uint32_t) uvaia_gpu_db_side_row_ints () || set->tile_bytes != uvaia_gpu_db_tile_bytes (gpu))) biomcmc_error ("packed database %s does not match this engine's tile layout", in[0]);
  unpack_out out = {prefix ? biomcmc_open_compress (outfilename, "w") : NULL, 0};
  uvdb_extract_stats st;
  memset (&st, 0, sizeof st);
  if (n) {
    if (uvdb_extract (set, gpu, pos, n, unpack_record, &out, &st, msg, sizeof msg)) biomcmc_error ("--unpack: %s", msg);
    uvaia_gpu_close (gpu);
  }
  if (out.xz) biomcmc_close_compress (out.xz);
  else if (fflush (stdout)) biomcmc_error ("--unpack: problem writing to standard output");
  fprintf (stderr, "Unpacked %llu of %llu sequences (%u sites) from %d packed database%s to %s in %.3lf secs.\n", (unsigned long long) n, (unsigned long long) set->n_ref, set->nchar, n_in,
           n_in > 1 ? "s" : "", prefix ? outfilename : "standard output", biomcmc_update_elapsed_time (time0));
  fprintf (stderr, "unpack report: {\"rows\": %llu, \"chunks\": %llu, \"stage_calls\": %llu, \"tiles_staged\": %llu, \"stage_ms\": %.3f, \"decode_ms\": %.3f, \"decode_kernel_ms\": %.3f, \"exceptions_ms\": %.3f, \"write_ms\": %.3f}\n",
           (unsigned long long) st.n_rows, (unsigned long long) st.n_chunks, (unsigned long long) st.n_pieces, (unsigned long long) st.n_tiles, st.stage_ms, st.decode_ms, st.kernel_ms, st.exceptions_ms, st.write_ms);
  if (names) {
    size_t absent = 0;
    for (size_t k = 0; k < names->n; k++) if (!names->hits[k]) absent++;
    if (absent) fprintf (stderr, "%zu of the %zu names in %s match no reference:\n", absent, names->n, names_file);
    for (size_t k = 0; k < names->n; k++) if (!names->hits[k]) fprintf (stderr, "  %s\n", names->name[k]);
  }
  uvdb_name_list_free (names);
  uvdb_set_close (set);
  free (pos); free (outfilename);
  return EXIT_SUCCESS;
}

/* `uvaiapack --merge`.  Whole tiles are exported once MERGE_BATCH references are resident and dropped from the front of the resident
 * database (uvaia_gpu_db_drop_tiles); the partly filled last tile stays resident and the next input's references go on filling it. */
static int
merge_main (int n_in, char **in, const char *out, int have_ambig, double ambig_r, int device, int compact)
{
  enum { MERGE_BATCH = PACK_BATCH, CHUNK_TILES = PACK_BATCH / 64 };
  char msg[1024];
  int64_t time0[2];
  biomcmc_get_time (time0);
  if (n_in > UVDB_SET_MAX_FILES) biomcmc_error ("--merge: at most %d packed databases", UVDB_SET_MAX_FILES);
  uvdb_set set = uvdb_set_open ((const char *const *) in, n_in, have_ambig ? UVDB_SET_ANY_AMBIGUITY : 0, msg, sizeof msg);
  if (!set) biomcmc_error ("%s", msg);
  if (!have_ambig) ambig_r = set->ref_ambiguity;
  for (int f = 0; f < n_in; f++) if (ambig_r > set->db[f]->h.ref_ambiguity)
    biomcmc_error ("--merge: -A %g is looser than the -A %g that packed database %s was filtered with: it does not hold the rows that filter dropped", ambig_r, set->db[f]->h.ref_ambiguity, in[f]);
  const int nchar = (int) set->nchar, non_n_ref = (int) (nchar * (1. - ambig_r));      /* the threshold of the text path below */
  if (compact && nchar > UVDB_COMPACT_MAX_NCHAR) biomcmc_error ("--compact: alignments of more than %d sites have no compact form (%d sites)", UVDB_COMPACT_MAX_NCHAR, nchar);

  uvaia_gpu_ctx *gpu = open_engine (nchar, device);
  const size_t tb = uvaia_gpu_db_tile_bytes (gpu), row = (size_t) uvaia_gpu_db_side_row_ints ();
  if (set->tile_bytes != tb || set->side_row_ints != (uint32_t) row) biomcmc_error ("packed database %s does not match this engine's tile layout", in[0]);
  /* resident: what a round leaves behind (below MERGE_BATCH) and one chunk on top of it */
  if (uvaia_gpu_db_reserve (gpu, 2 * MERGE_BATCH) || uvaia_gpu_db_stage_reserve (gpu, CHUNK_TILES)) biomcmc_error ("%s", uvaia_gpu_last_error (gpu));
  struct uvdb_export exp;
  memset (&exp, 0, sizeof exp);
  int *sel = (int *) biomcmc_malloc (MERGE_BATCH * sizeof (int));
  uvdb_writer w = compact ? uvdb_create_compact (out, nchar, tb, (int) row, ambig_r) : uvdb_create (out, nchar, tb, (int) row, ambig_r);
  if (!w) biomcmc_error ("cannot create %s", out);
  long count = 0, kept = 0;
  int slot = 0;
  for (int f = 0; f <= n_in; f++) {
    uvdb_reader db = f < n_in ? set->db[f] : NULL;
    const int filter = db && ambig_r < db->h.ref_ambiguity;      /* only then can a stored row fall below the threshold */
    for (uint64_t t = 0; db && t < db->h.n_tiles; t += CHUNK_TILES) {
      const uint64_t nt = db->h.n_tiles - t < CHUNK_TILES ? db->h.n_tiles - t : CHUNK_TILES;
      const uint64_t r0 = t * 64, r1 = r0 + nt * 64 < db->h.n_ref ? r0 + nt * 64 : db->h.n_ref;
      int m = 0;
      for (uint64_t r = r0; r < r1; r++) {
        count++;
        if (filter && db->non_n[r] < non_n_ref) continue;
        if (uvdb_add_reference_runs (w, uvdb_name (db, r), db->exc + db->exc_idx[r], (size_t) (db->exc_idx[r + 1] - db->exc_idx[r]))) biomcmc_error ("out of memory while indexing %s", uvdb_name (db, r));
        sel[m++] = (int) (r - r0);
      }
      kept += m;
      if (!m) continue;
      const uvdb_set_piece piece = {f, t, nt, 0};          /* the chunk's tiles as one piece at the start of the slot, dense or compact */
      if (uvdb_stage_pieces (gpu, set, slot, &piece, 1) ||
          uvaia_gpu_db_append_staged (gpu, slot, (uint64_t) m == r1 - r0 ? NULL : sel, m)) biomcmc_error ("%s", uvaia_gpu_last_error (gpu));
      slot ^= 1;
      const size_t whole = uvaia_gpu_db_size (gpu) / 64;
      if (uvaia_gpu_db_size (gpu) >= MERGE_BATCH) {
        if (uvdb_export_tiles (&exp, gpu, w, 0, whole)) biomcmc_error ("%s: %s", out, exp.err);
        if (uvaia_gpu_db_drop_tiles (gpu, whole)) biomcmc_error ("%s", uvaia_gpu_last_error (gpu));
      }
    }
    if (db) fprintf (stderr, "Finished merging file %s in %.3lf secs; %ld sequences so far, %ld kept.\n", in[f], biomcmc_update_elapsed_time (time0), count, kept);
    else if (uvaia_gpu_db_size (gpu)) {                  /* the tail after the last input */
      const size_t nt = (uvaia_gpu_db_size (gpu) + 63) / 64;
      if (uvdb_export_tiles (&exp, gpu, w, 0, nt)) biomcmc_error ("%s: %s", out, exp.err);
    }
  }
  if (uvdb_close (w)) biomcmc_error ("problem writing %s", out);
  fprintf (stderr, "Merged %ld of %ld sequences (%d sites, -A %g) from %d packed databases into %s", kept, count, nchar, ambig_r, n_in, out);
  if (compact) fprintf (stderr, "; compact tiles: %ld encoded on the device, %ld on the host", exp.tiles_device, exp.tiles_host);
  fprintf (stderr, "\n");
  uvaia_gpu_close (gpu);
  uvdb_set_close (set);
  uvdb_export_free (&exp);
  free (sel);
  return EXIT_SUCCESS;
}

/* `uvaiapack --device-parse`.  The first record of the first file fixes the alignment length and opens the packer; rows of that length go
 * to it as they lie in device memory, a record of another length is treated as on the default route (pack_main.c, the fill loop of main):
 * dropped as too ambiguous, or the end of the command. */
#define PARSE_MAX_RECORDS (1 << 18)     /* records per scan: 8 MiB of table; a block that holds more is scanned in several steps */

struct device_parse {
  uvaia_gpu_fasta *fasta;
  struct uvdb_packer packer;
  int open, nchar, non_n_ref, compact, device, max_records;
  double ambig_r;
  const char *out;
  uvaia_gpu_fasta_record *rec;
  int *row_of;
  char **name;
  long count, n_other_dropped;
};

static int
parse_scan (void *user, const char *text, size_t n, int final, int *n_records, size_t *consumed, int *bad_kind, size_t *bad_off, char *err, size_t errlen)
{
  struct device_parse *d = (struct device_parse *) user;
  if (!uvaia_gpu_fasta_scan (d->fasta, text, n, final, n_records, consumed)) return 0;
  const unsigned kind = uvaia_gpu_fasta_bad (d->fasta, bad_off);       /* irregular text: the block reader names the byte of the stream */
  *bad_kind = kind == UVAIA_GPU_FASTA_NUL ? FASTA_BAD_NUL : kind == UVAIA_GPU_FASTA_TEXT ? FASTA_BAD_TEXT : kind == UVAIA_GPU_FASTA_EMPTY ? FASTA_BAD_EMPTY : FASTA_BAD_NONE;
  snprintf (err, errlen, "%s", uvaia_gpu_fasta_last_error (d->fasta));
  return -1;
}

static int
parse_records (void *user, char *text, size_t consumed, int n_records, char *err, size_t errlen)
{
  struct device_parse *d = (struct device_parse *) user;
  if (uvaia_gpu_fasta_records (d->fasta, d->rec)) { snprintf (err, errlen, "%s", uvaia_gpu_fasta_last_error (d->fasta)); return -1; }
  if (!d->open) {       /* the first record fixes the alignment length */
    d->nchar = (int) d->rec[0].seq_len;
    d->non_n_ref = (int) (d->nchar * (1. - d->ambig_r));
    if (uvdb_packer_open (&d->packer, d->out, d->nchar, d->ambig_r, d->device, d->max_records, d->compact)) { snprintf (err, errlen, "%s", d->packer.err); return -1; }
    d->open = 1;
  }
  const void *d_rows = NULL; size_t pitch = 0; int n_rows = 0;
  if (uvaia_gpu_fasta_rows (d->fasta, d->nchar, &d_rows, &pitch, &n_rows, d->row_of)) { snprintf (err, errlen, "%s", uvaia_gpu_fasta_last_error (d->fasta)); return -1; }
  d->count += n_records;
  for (int k = 0; k < n_records; k++) {
    const uvaia_gpu_fasta_record *r = d->rec + k;
    text[r->name_off + r->name_len] = '\0';              /* the line end behind the name, or the byte of room behind the block */
    if (d->row_of[k] >= 0) { d->name[d->row_of[k]] = text + r->name_off; continue; }
    /* as the reference's fill loop (src/nearest.c:263-278): low-quality records are dropped first, only then must the length fit */
    if (r->non_n < d->non_n_ref) { d->n_other_dropped++; continue; }
    biomcmc_warning ("Reference sequence '%s' has %u sites but the first sequence has %d sites\n", text + r->name_off, r->seq_len, d->nchar);
    snprintf (err, errlen, "all sequences must be aligned");
    return -1;
  }
  if (n_rows && uvdb_packer_add_block (&d->packer, d_rows, pitch, n_rows, d->name)) { snprintf (err, errlen, "%s", d->packer.err); return -1; }
  return 0;
}

static int
device_parse_main (int n_in, char **in, const char *out, double ambig_r, int device, int compact, size_t block_bytes)
{
  char msg[1024];
  int64_t time0[2];
  biomcmc_get_time (time0);
  struct device_parse d;
  memset (&d, 0, sizeof d);
  d.ambig_r = ambig_r; d.device = device; d.compact = compact; d.out = out;
  d.max_records = block_bytes / 4 + 1 < PARSE_MAX_RECORDS ? (int) (block_bytes / 4 + 1) : PARSE_MAX_RECORDS;      /* (a record has four bytes at least) */
  if (uvaia_gpu_fasta_open (&d.fasta, device, block_bytes, d.max_records)) biomcmc_error ("%s", uvaia_gpu_fasta_last_error (NULL));
  d.rec = (uvaia_gpu_fasta_record *) biomcmc_malloc ((size_t) d.max_records * sizeof (uvaia_gpu_fasta_record));
  d.row_of = (int *) biomcmc_malloc ((size_t) d.max_records * sizeof (int));
  d.name = (char **) biomcmc_malloc ((size_t) d.max_records * sizeof (char *));
  uint64_t bytes = 0;
  for (int j = 0; j < n_in; j++) {
    uint64_t nb = 0;
    fasta_blocks fb = fasta_blocks_open (in[j], block_bytes, uvaia_gpu_fasta_pinned_alloc, uvaia_gpu_fasta_pinned_free, msg, sizeof msg);
    int rc = fb ? fasta_blocks_run (fb, d.max_records, parse_scan, &d, parse_records, &d, &nb, msg, sizeof msg) : -1;
    if (rc && d.open) remove (out);                           /* no output file is left behind, whatever ends the command */
    char failed[1024];                                        /* a decompressor that failed mid-stream: what was read is not the file, and */
    if (fasta_blocks_finish (fb, failed, sizeof failed)) {    /* what its cut end looked like (a short last record) is not the finding */
      if (d.open) remove (out);
      biomcmc_error ("%s", failed);
    }
    if (rc) {
      const int text = strstr (msg, "FASTA text:") || strstr (msg, "does not fit a block");     /* what the parser refuses, the line reader takes */
      biomcmc_error ("%s%s", msg, text ? " (--device-parse takes regular FASTA whose records fit a block: `uvaiapack` without it reads this file line by line)" : "");
    }
    bytes += nb;
    fprintf (stderr, "Finished reading file %s in %.3lf secs; %ld sequences so far, %ld kept, %ld too ambiguous.\n", in[j], biomcmc_update_elapsed_time (time0), d.count,
             d.open ? d.packer.kept : 0L, d.n_other_dropped + (d.open ? d.packer.dropped : 0L));
  }
  if (!d.open) biomcmc_error ("no sequence found");
  const long kept = d.packer.kept;
  if (uvdb_packer_close (&d.packer)) { remove (out); biomcmc_error ("%s: %s", out, d.packer.err); }
  double ms[2] = {0., 0.};
  uvaia_gpu_fasta_kernel_ms (d.fasta, ms, 0);
  fprintf (stderr, "device parse: {\"bytes\": %llu, \"block_bytes\": %zu, \"scan_ms\": %.3f, \"rows_ms\": %.3f, \"scan_gb_s\": %.2f, \"rows_gb_s\": %.2f}\n", (unsigned long long) bytes, block_bytes, ms[0], ms[1],
           ms[0] > 0 ? (double) bytes / ms[0] * 1e-6 : 0., ms[1] > 0 ? (double) bytes / ms[1] * 1e-6 : 0.);
  fprintf (stderr, "Packed %ld of %ld sequences (%d sites) into %s", kept, d.count, d.nchar, out);
  if (compact) fprintf (stderr, "; compact tiles: %ld encoded on the device, %ld on the host", d.packer.tiles_device, d.packer.tiles_host);
  fprintf (stderr, "\n");
  uvaia_gpu_fasta_close (d.fasta);
  free (d.rec); free (d.row_of); free (d.name);
  return EXIT_SUCCESS;
}

int
main (int argc, char **argv)
{
  double ambig_r = 0.5;
  const char *out = NULL, *names_file = NULL;
  int device = -1, ch, errors = 0, merge = 0, have_ambig = 0, compact = 0, unpack = 0, to_stdout = 0, list = 0, device_parse = 0;
  size_t parse_block = FASTA_BLOCK_BYTES;
  static const struct option longopts[] = {{"help", no_argument, 0, 'h'}, {"version", no_argument, 0, 'v'}, {"ref_ambiguity", required_argument, 0, 'A'},
    {"output", required_argument, 0, 'o'}, {"device", required_argument, 0, 1002}, {"merge", no_argument, 0, 1003}, {"compact", no_argument, 0, 1004},
    {"unpack", no_argument, 0, 1005}, {"stdout", no_argument, 0, 1006}, {"names", required_argument, 0, 1007}, {"list", no_argument, 0, 1008},
    {"device-parse", no_argument, 0, 1009}, {"parse-block", required_argument, 0, 1010}, {0, 0, 0, 0}};
  while ((ch = getopt_long (argc, argv, "hvA:o:", longopts, NULL)) != -1) switch (ch) {
    case 'h': usage (basename (argv[0])); return EXIT_SUCCESS;
    case 'v': printf ("%s\n", UVAIA_PACKAGE_VERSION); return EXIT_SUCCESS;
    case 'A': ambig_r = atof (optarg); have_ambig = 1; break;
    case 'o': out = optarg; break;
    case 1002: device = atoi (optarg); break;
    case 1003: merge = 1; break;
    case 1004: compact = 1; break;
    case 1005: unpack = 1; break;
    case 1006: to_stdout = 1; break;
    case 1007: names_file = optarg; break;
    case 1008: list = 1; break;
    case 1009: device_parse = 1; break;
    case 1010: parse_block = (size_t) strtoull (optarg, NULL, 10); break;      /* (for tests: the block size of --device-parse in bytes) */
    default: errors++;
  }
  /* what does not go together is refused here, before a file is opened or a GPU touched */
  if (device_parse && (merge || unpack || list)) { fprintf (stderr, "--device-parse reads FASTA text: it does not go with --merge, --unpack or --list\n"); return EXIT_FAILURE; }
  if (device_parse && (parse_block < 64 || parse_block > ((size_t) 1 << 30))) { fprintf (stderr, "--parse-block: expected 64 to 1073741824 bytes\n"); return EXIT_FAILURE; }
  if (!device_parse && parse_block != FASTA_BLOCK_BYTES) { fprintf (stderr, "--parse-block sets the block size of --device-parse: it needs that option\n"); return EXIT_FAILURE; }
  if (list && (unpack || merge || compact || have_ambig || out || to_stdout || names_file)) { fprintf (stderr, "--list prints the stored names and takes no other option\n"); return EXIT_FAILURE; }
  if (unpack && (merge || compact || have_ambig)) { fprintf (stderr, "--unpack writes the references as they are stored: it does not go with --merge, --compact or -A\n"); return EXIT_FAILURE; }
  if (unpack && !errors && (!out) == (!to_stdout)) { fprintf (stderr, "--unpack needs exactly one of -o <prefix> and --stdout\n"); return EXIT_FAILURE; }
  if (names_file && !unpack) { fprintf (stderr, "--names needs --unpack: it chooses the references that are written\n"); return EXIT_FAILURE; }
  if (to_stdout && !unpack) { fprintf (stderr, "--stdout needs --unpack\n"); return EXIT_FAILURE; }
  if (!errors && optind < argc && list) return list_main (argc - optind, argv + optind);
  if (!errors && optind < argc && unpack) return unpack_main (argc - optind, argv + optind, out, names_file, device);
  if (list || unpack) out = NULL;                      /* (no input given: the usage below) */
  if (errors || !out || optind >= argc) { printf ("Error when reading arguments from command line:\n"); usage (basename (argv[0])); return EXIT_FAILURE; }
  if (ambig_r < 0.001) ambig_r = 0.001;
  if (ambig_r > 1.) ambig_r = 1.;
  if (merge) return merge_main (argc - optind, argv + optind, out, have_ambig, ambig_r, device, compact);
  if (device_parse) return device_parse_main (argc - optind, argv + optind, out, ambig_r, device, compact, parse_block);
  int64_t time0[2];
  biomcmc_get_time (time0);

  uvaia_gpu_ctx *gpu = NULL;
  uvdb_writer w = NULL;
  char **seq = (char **) biomcmc_malloc (PACK_BATCH * sizeof (char *));
  int *non_n = (int *) biomcmc_malloc (PACK_BATCH * sizeof (int));
  struct uvdb_export exp;
  memset (&exp, 0, sizeof exp);
  int nchar = 0, non_n_ref = 0, fill = 0;
  long count = 0, kept = 0, n_invalid = 0;

  for (int j = optind; j <= argc; j++) {
    readfasta_t rfas = j < argc ? new_readfasta (argv[j]) : NULL;
    for (;;) {
      const int have = rfas ? (readfasta_next (rfas) >= 0) : 0;
      if (have) {
        count++;
        if (!gpu) {       /* the first record fixes the alignment length */
          nchar = (int) rfas->seqlength;
          non_n_ref = (int) (nchar * (1. - ambig_r));
          gpu = open_engine (nchar, device);
          if (uvaia_gpu_db_reserve (gpu, PACK_BATCH)) biomcmc_error ("%s", uvaia_gpu_last_error (gpu));
          const size_t tb = uvaia_gpu_db_tile_bytes (gpu);
          if (compact && nchar > UVDB_COMPACT_MAX_NCHAR) biomcmc_error ("--compact: alignments of more than %d sites have no compact form (%d sites)", UVDB_COMPACT_MAX_NCHAR, nchar);
          w = compact ? uvdb_create_compact (out, nchar, tb, uvaia_gpu_db_side_row_ints (), ambig_r) : uvdb_create (out, nchar, tb, uvaia_gpu_db_side_row_ints (), ambig_r);
          if (!w) biomcmc_error ("cannot create %s", out);
        }
        /* as the reference's fill loop (src/nearest.c:263-278): low-quality records are dropped first, only then must the length fit */
        const int nn = quick_count_sequence_non_N (rfas->seq, rfas->seqlength);
        if (nn < non_n_ref) { n_invalid++; continue; }
        if (rfas->seqlength != (size_t) nchar) {
          biomcmc_warning ("Reference sequence '%s' has %zu sites but the first sequence has %d sites\n", rfas->name, rfas->seqlength, nchar);
          biomcmc_error ("all sequences must be aligned");
        }
        if (uvdb_add_reference (w, rfas->name, rfas->seq)) biomcmc_error ("out of memory while indexing %s", rfas->name);
        non_n[fill] = nn;
        seq[fill++] = rfas->seq; rfas->seq = NULL;
        kept++;
      }
      if (fill == PACK_BATCH || (!have && j == argc && fill)) {     /* a full batch, or the tail after the last file */
        const size_t nt = ((size_t) fill + 63) / 64;
        if (uvaia_gpu_db_append (gpu, (const char *const *) seq, non_n, fill)) biomcmc_error ("%s", uvaia_gpu_last_error (gpu));
        if (uvdb_export_tiles (&exp, gpu, w, 0, nt)) biomcmc_error ("%s: %s", out, exp.err);
        if (uvaia_gpu_db_clear (gpu)) biomcmc_error ("%s", uvaia_gpu_last_error (gpu));
        for (int c = 0; c < fill; c++) free (seq[c]);
        fill = 0;
      }
      if (!have) break;
    }
    if (rfas) {
      del_readfasta (rfas);
      fprintf (stderr, "Finished reading file %s in %.3lf secs; %ld sequences so far, %ld kept, %ld too ambiguous.\n", argv[j], biomcmc_update_elapsed_time (time0), count, kept, n_invalid);
    }
  }
  if (!w) biomcmc_error ("no sequence found");
  if (uvdb_close (w)) biomcmc_error ("problem writing %s", out);
  fprintf (stderr, "Packed %ld of %ld sequences (%d sites) into %s", kept, count, nchar, out);
  if (compact) fprintf (stderr, "; compact tiles: %ld encoded on the device, %ld on the host", exp.tiles_device, exp.tiles_host);
  fprintf (stderr, "\n");
  uvaia_gpu_close (gpu);
  uvdb_export_free (&exp);
  free (seq); free (non_n);
  return EXIT_SUCCESS;
}
