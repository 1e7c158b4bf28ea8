/*
 * align_main.c -- `uvaialign`: aligns query sequences against one reference sequence and writes them on the reference's
 * columns.  Same options, filters, messages and output as the reference's src/align.c; the per-pool loop over align_query
 * (src/align.c:224-233,357-390) runs on the GPU through include/uvaia_align.h.
 *
 * --packed (no counterpart in the reference): the aligned rows go from the aligner's device memory straight into a packed database
 * (uvdb.h), the file `uvaiapack` would write from the text output: census, -A filter, packing and exception runs happen on the rows where
 * they lie (include/uvaia_gpu.h, "rows that are already in device memory").  Own code.
 *
 * --device-parse (no counterpart either, off by default): the input is split into sequences on the GPU and handed to the aligner in device
 * memory, see align_device_parse below.  Without the option the command takes the read loop of main as it was.
 *
 * --insertions (no counterpart either): the characters the projection drops (the I operations of src/align.c:366-390) go to a table, one
 * line per insertion run, from the records the aligner keeps (include/uvaia_align.h, uvaia_align_fetch_insertions).
 *
 * --variants, --qc (no counterpart either): what every aligned row differs from the reference by -- substitutions and deletions, which the
 * aligner derives from the rows where they lie (uvaia_align_set_variants), merged with the insertion runs -- and one line of counts per
 * aligned sequence.
 */
#define _GNU_SOURCE
#include <getopt.h>
#include <inttypes.h>
#include <libgen.h>
#include <omp.h>

#include "cli_common.h"
#include "fastaseq.h"
#include "gpu_glue.h"
#include "uvdb.h"
#include "uvdb_packer.h"
#include "fasta_blocks.h"
#include "../../../include/uvaia_align.h"
#include "../../../include/uvaia_gpu.h"

/* one pool into the packed database in the making: the rows of the aligner's last run, where they lie */
static int
packer_add_pool (struct uvdb_packer *p, uvaia_aligner *al, char **name, int fill)
{
  const void *d_rows = NULL; size_t pitch = 0; int n = 0;
  if (uvaia_align_device_rows (al, &d_rows, &pitch, &n, NULL)) { snprintf (p->err, sizeof p->err, "%s", uvaia_align_last_error (al)); return -1; }
  if (n != fill) { snprintf (p->err, sizeof p->err, "the aligner holds %d rows, the pool %d", n, fill); return -1; }
  return uvdb_packer_add_block (p, d_rows, pitch, n, name);
}

/* `uvaialign --insertions <file>`: sequence,ref_pos,length,bases for every insertion run of every aligned sequence, in the order the
 * sequences are written and by ref_pos within one; names go out raw, as the search's table writes them */
struct ins_table {
  file_compress_t out;                  /* NULL without --insertions */
  long n_seqs; long long n_bases;
  uvaia_align_insertion *rec; char *bases, *line;
  size_t rec_cap, bases_cap, line_cap;
  char err[512];
};

static void
ins_table_open (struct ins_table *t, const char *filename)
{
  static const char header[] = "sequence,ref_pos,length,bases\n";
  memset (t, 0, sizeof *t);
  if (!filename) return;
  t->out = biomcmc_open_compress (filename, "w");
  if (biomcmc_write_compress (t->out, header) != (int) strlen (header)) fprintf (stderr, "File %s may not be correctly compressed: its first line could not be written.\n", filename);
}

static void
ins_table_close (struct ins_table *t)
{
  if (t->out) biomcmc_close_compress (t->out);
  free (t->rec); free (t->bases); free (t->line);
  t->out = NULL; t->rec = NULL; t->bases = NULL; t->line = NULL;
}

/* the runs of the aligner's last run: its queries are name[0 ..] */
static int
ins_table_add (struct ins_table *t, uvaia_aligner *al, char **name)
{
  long long n_rec = 0, n_bases = 0;
  if (!t->out) return 0;
  if (uvaia_align_insertion_counts (al, &n_rec, &n_bases)) { snprintf (t->err, sizeof t->err, "%s", uvaia_align_last_error (al)); return -1; }
  if (!n_rec) return 0;
  if ((size_t) n_rec > t->rec_cap) { t->rec_cap = (size_t) n_rec * 2; t->rec = (uvaia_align_insertion *) biomcmc_realloc (t->rec, t->rec_cap * sizeof (uvaia_align_insertion)); }
  if ((size_t) n_bases > t->bases_cap) { t->bases_cap = (size_t) n_bases * 2; t->bases = (char *) biomcmc_realloc (t->bases, t->bases_cap); }
  if (uvaia_align_fetch_insertions (al, t->rec, t->bases)) { snprintf (t->err, sizeof t->err, "%s", uvaia_align_last_error (al)); return -1; }
  int bad = 0;
  size_t at = 0;
  for (long long r = 0; r < n_rec; r++) {
    const uvaia_align_insertion *c = t->rec + r;
    const char *nm = name[c->query];
    const size_t need = strlen (nm) + (size_t) c->length + 64;
    if (need > t->line_cap) { t->line_cap = need * 2; t->line = (char *) biomcmc_realloc (t->line, t->line_cap); }
    int w = snprintf (t->line, t->line_cap, "%s,%d,%d,", nm, c->ref_pos, c->length);
    memcpy (t->line + w, t->bases + at, (size_t) c->length);
    w += c->length;
    t->line[w++] = '\n'; t->line[w] = '\0';
    bad += biomcmc_write_compress (t->out, t->line) != w;
    at += (size_t) c->length;
    if (!r || c[-1].query != c->query) t->n_seqs++;
  }
  t->n_bases += n_bases;
  if (bad) fprintf (stderr, "File %s may not be correctly compressed, %d error%s occurred when saving insertions.\n", t->out->filename, bad, bad > 1 ? "s" : "");
  return 0;
}

/* `uvaialign --variants <file>`: sequence,kind,ref_pos,length,ref,alt -- S (ref and alt bytes), D (both empty) and I (the inserted bases in
 * alt) of every aligned sequence, in the order the sequences are written and by ref_pos within one; at equal ref_pos the I goes first, since
 * it lies left of that site.  `--qc <file>`: one line of counts per aligned sequence.  Either file may be absent. */
struct var_table {
  file_compress_t variants, qc;         /* NULL without the option */
  long n_seqs; long long n_sub, n_del, n_del_sites, n_ins, n_ins_bases;
  uvaia_align_variant *rec; uvaia_align_row_qc *row; uvaia_align_insertion *ins; char *bases, *line; int *score;
  size_t rec_cap, row_cap, ins_cap, bases_cap, line_cap;
  int bad;
  char err[512];
};

static void
var_table_open (struct var_table *t, const char *variants, const char *qc)
{
  static const char head_v[] = "sequence,kind,ref_pos,length,ref,alt\n";
  static const char head_q[] = "sequence,length,score,matches,substitutions,deletions,deleted_sites,insertions,inserted_bases,unknown_sites,other_sites,first_site,last_site\n";
  memset (t, 0, sizeof *t);
  if (variants) {
    t->variants = biomcmc_open_compress (variants, "w");
    if (biomcmc_write_compress (t->variants, head_v) != (int) strlen (head_v)) fprintf (stderr, "File %s may not be correctly compressed: its first line could not be written.\n", variants);
  }
  if (qc) {
    t->qc = biomcmc_open_compress (qc, "w");
    if (biomcmc_write_compress (t->qc, head_q) != (int) strlen (head_q)) fprintf (stderr, "File %s may not be correctly compressed: its first line could not be written.\n", qc);
  }
}

static void
var_table_close (struct var_table *t)
{
  if (t->variants) biomcmc_close_compress (t->variants);
  if (t->qc) biomcmc_close_compress (t->qc);
  free (t->rec); free (t->row); free (t->ins); free (t->bases); free (t->line); free (t->score);
  t->variants = t->qc = NULL; t->rec = NULL; t->row = NULL; t->ins = NULL; t->bases = NULL; t->line = NULL; t->score = NULL;
}

/* the aligner's last run: its queries are name[0 ..], len[0 ..] characters long */
static int
var_table_add (struct var_table *t, uvaia_aligner *al, char **name, const int *len)
{
  long long n_rec = 0, n_ins = 0, n_bases = 0;
  int n_rows = 0;
  if (!t->variants && !t->qc) return 0;
  if (uvaia_align_variant_counts (al, &n_rec, &n_rows) || uvaia_align_insertion_counts (al, &n_ins, &n_bases)) { snprintf (t->err, sizeof t->err, "%s", uvaia_align_last_error (al)); return -1; }
  if (!n_rows) return 0;
  if ((size_t) n_rec > t->rec_cap) { t->rec_cap = (size_t) n_rec * 2; t->rec = (uvaia_align_variant *) biomcmc_realloc (t->rec, t->rec_cap * sizeof (uvaia_align_variant)); }
  if ((size_t) n_rows > t->row_cap) {
    t->row_cap = (size_t) n_rows * 2;
    t->row = (uvaia_align_row_qc *) biomcmc_realloc (t->row, t->row_cap * sizeof (uvaia_align_row_qc));
    t->score = (int *) biomcmc_realloc (t->score, t->row_cap * sizeof (int));
  }
  if ((size_t) n_ins > t->ins_cap) { t->ins_cap = (size_t) n_ins * 2; t->ins = (uvaia_align_insertion *) biomcmc_realloc (t->ins, t->ins_cap * sizeof (uvaia_align_insertion)); }
  if ((size_t) n_bases > t->bases_cap) { t->bases_cap = (size_t) n_bases * 2; t->bases = (char *) biomcmc_realloc (t->bases, t->bases_cap); }
  if (uvaia_align_fetch_variants (al, t->rec, t->row) || uvaia_align_fetch_insertions (al, t->ins, t->bases) || uvaia_align_fetch (al, NULL, t->score)) {
    snprintf (t->err, sizeof t->err, "%s", uvaia_align_last_error (al));
    return -1;
  }
  long long iv = 0, ii = 0;
  size_t at = 0;
  int bad = 0;
  for (int q = 0; q < n_rows; q++) {     /* both lists are sorted by (query, ref_pos): one merge per sequence */
    const uvaia_align_row_qc *c = t->row + q;
    const char *nm = name[q];
    const size_t nm_len = strlen (nm);
    int q_ins = 0;
    long long q_bases = 0;
    for (;;) {
      const int has_v = iv < n_rec && t->rec[iv].query == q, has_i = ii < n_ins && t->ins[ii].query == q;
      if (!has_v && !has_i) break;
      const int take_i = has_i && (!has_v || t->ins[ii].ref_pos <= t->rec[iv].ref_pos);
      const size_t need = nm_len + 96 + (take_i ? (size_t) t->ins[ii].length : 0);
      if (need > t->line_cap) { t->line_cap = need * 2; t->line = (char *) biomcmc_realloc (t->line, t->line_cap); }
      int w;
      if (take_i) {
        const uvaia_align_insertion *r = t->ins + ii++;
        w = snprintf (t->line, t->line_cap, "%s,I,%d,%d,,", nm, r->ref_pos, r->length);
        memcpy (t->line + w, t->bases + at, (size_t) r->length);
        w += r->length; at += (size_t) r->length;
        q_ins++; q_bases += r->length;
      } else {
        const uvaia_align_variant *r = t->rec + iv++;
        const int kind = (int) (r->kind_ref_alt & 0xFF);
        if (kind == 'S') w = snprintf (t->line, t->line_cap, "%s,S,%d,%d,%c,%c", nm, r->ref_pos, r->length, (int) ((r->kind_ref_alt >> 8) & 0xFF), (int) ((r->kind_ref_alt >> 16) & 0xFF));
        else w = snprintf (t->line, t->line_cap, "%s,%c,%d,%d,,", nm, kind, r->ref_pos, r->length);
      }
      t->line[w++] = '\n'; t->line[w] = '\0';
      if (t->variants) bad += biomcmc_write_compress (t->variants, t->line) != w;
    }
    if (t->qc) {
      if (nm_len + 256 > t->line_cap) { t->line_cap = (nm_len + 256) * 2; t->line = (char *) biomcmc_realloc (t->line, t->line_cap); }
      const int w = snprintf (t->line, t->line_cap, "%s,%d,%d,%d,%d,%d,%d,%d,%lld,%d,%d,%d,%d\n", nm, len[q], t->score[q], c->matches, c->substitutions, c->deletion_runs, c->deleted_sites, q_ins, q_bases,
                              c->unknown_sites, c->other_sites, c->first_site, c->last_site);
      bad += biomcmc_write_compress (t->qc, t->line) != w;
    }
    t->n_seqs++;
    t->n_sub += c->substitutions; t->n_del += c->deletion_runs; t->n_del_sites += c->deleted_sites; t->n_ins += q_ins; t->n_ins_bases += q_bases;
  }
  if (iv != n_rec || ii != n_ins) { snprintf (t->err, sizeof t->err, "records of a sequence the pool does not hold, or out of order (%lld of %lld variants, %lld of %lld insertions taken)", iv, n_rec, ii, n_ins); return -1; }
  if (bad) fprintf (stderr, "The variant or QC table may not be correctly compressed, %d error%s occurred when saving %d sequences.\n", bad, bad > 1 ? "s" : "", n_rows);
  return 0;
}

/* `uvaialign --device-parse`: the text is read in blocks (fasta_blocks.h) and split into records on the GPU (uvaia_gpu_fasta_scan); the
 * filters of the fill loop in main run on the integers of the record table and the A C G T counts; the survivors of a scan go, a pool at a
 * time and in record order, from the parser's device memory into the aligner's (uvaia_gpu_fasta_sequences, uvaia_align_load_device).  Only
 * the names are taken from the host's copy of the text.  The reader thread fills the next block while this one is aligned. */
#define PARSE_MAX_RECORDS (1 << 18)     /* records per scan, as in pack_main.c; a block that holds more is scanned in several steps */

struct align_parse {
  uvaia_gpu_fasta *fasta;
  uvaia_aligner *al;
  struct uvdb_packer *pk;               /* NULL without --packed */
  struct ins_table *ins;
  struct var_table *var;
  int *len;                             /* main's array of a pool: the queries' lengths, for the QC table */
  file_compress_t outstream;
  bool to_screen, write_text;
  size_t aln_length;
  double ambig, align_ms;
  int pool, count, n_output, n_pool;
  uvaia_gpu_fasta_record *rec;          /* max_records of each */
  int *acgt, *sel;
  int64_t *offsets;                     /* pool + 1 */
  char **name, *aln;                    /* main's arrays of a pool */
  int64_t *time1;
};

static int
align_parse_scan (void *user, const char *text, size_t n, int final, int *n_records, size_t *consumed, int *bad_kind, size_t *bad_off, char *err, size_t errlen)
{
  struct align_parse *d = (struct align_parse *) user;
  if (!uvaia_gpu_fasta_scan (d->fasta, text, n, final, n_records, consumed)) return 0;
  const unsigned kind = uvaia_gpu_fasta_bad (d->fasta, bad_off);       /* irregular text: the block reader names the byte of the stream */
  *bad_kind = kind == UVAIA_GPU_FASTA_NUL ? FASTA_BAD_NUL : kind == UVAIA_GPU_FASTA_TEXT ? FASTA_BAD_TEXT : kind == UVAIA_GPU_FASTA_EMPTY ? FASTA_BAD_EMPTY : FASTA_BAD_NONE;
  snprintf (err, errlen, "%s", uvaia_gpu_fasta_last_error (d->fasta));
  return -1;
}

static int
align_parse_records (void *user, char *text, size_t consumed, int n_records, char *err, size_t errlen)
{
  struct align_parse *d = (struct align_parse *) user;
  const size_t aln_length = d->aln_length;
  const double ambig = d->ambig;
  const int before = d->count;
  if (uvaia_gpu_fasta_records (d->fasta, d->rec) || uvaia_gpu_fasta_acgt (d->fasta, d->acgt)) { snprintf (err, errlen, "%s", uvaia_gpu_fasta_last_error (d->fasta)); return -1; }
  int n_sel = 0;
  for (int k = 0; k < n_records; k++) {               /* the filters of main's fill loop, on the counts the device made */
    const uvaia_gpu_fasta_record *r = d->rec + k;
    char *name = text + r->name_off;
    name[r->name_len] = '\0';                         /* the line end behind the name, or the byte of room behind the block */
    const size_t seqlength = r->seq_len;
    d->count++;
    if (((3 * seqlength) < (2 * aln_length)) || ((2 * seqlength) > (3 * aln_length))) {
      fprintf (stderr, "Sequence %s has size too different from reference (%lu vs %lu)\n", name, (unsigned long) seqlength, (unsigned long) aln_length);
      continue;
    }
    const double l = seqlength ? (double) seqlength : 1.;          /* biomcmc_count_sequence_acgt: [0] and [2] */
    const double frac_acgt = (double) d->acgt[k] / l, frac_bad = (double) ((size_t) r->seq_len - (size_t) r->non_n) / l;
    if (frac_bad > ambig) {
      fprintf (stderr, "Sequence %s has proportion of N etc. (=%lf) above threshold of %lf\n", name, frac_bad, ambig);
      continue;
    }
    if (frac_acgt < 1. - 1.1 * ambig) {
      fprintf (stderr, "Sequence %s has proportion of ACGT (=%lf) below threshold of %lf\n", name, frac_acgt, 1. - 1.1 * ambig);
      continue;
    }
    d->sel[n_sel++] = k;
  }
  for (int a = 0; a < n_sel; a += d->pool) {
    const int fill = n_sel - a < d->pool ? n_sel - a : d->pool;
    const void *d_bytes = NULL;
    double ms = 0.;
    d->n_pool++;
    for (int c = 0; c < fill; c++) d->name[c] = text + d->rec[d->sel[a + c]].name_off;
    if (uvaia_gpu_fasta_sequences (d->fasta, d->sel + a, fill, &d_bytes, d->offsets)) { snprintf (err, errlen, "%s", uvaia_gpu_fasta_last_error (d->fasta)); return -1; }
    if (uvaia_align_load_device (d->al, d_bytes, d->offsets, fill) || uvaia_align_run (d->al) || (d->write_text && uvaia_align_fetch (d->al, d->aln, NULL))) {
      snprintf (err, errlen, "%s (counted from sequence %s, the first of a pool of %d; %d sequences were written before)", uvaia_align_last_error (d->al), d->name[0], fill, d->n_output);
      return -1;
    }
    if (!uvaia_align_stats (d->al, NULL, NULL, NULL, &ms)) d->align_ms += ms;
    if (ins_table_add (d->ins, d->al, d->name)) {
      snprintf (err, errlen, "%s (insertions of the pool that starts with sequence %s; %d sequences were written before)", d->ins->err, d->name[0], d->n_output);
      return -1;
    }
    for (int c = 0; c < fill; c++) d->len[c] = (int) (d->offsets[c + 1] - d->offsets[c]);
    if (var_table_add (d->var, d->al, d->name, d->len)) {
      snprintf (err, errlen, "%s (variants of the pool that starts with sequence %s; %d sequences were written before)", d->var->err, d->name[0], d->n_output);
      return -1;
    }
    if (d->pk && packer_add_pool (d->pk, d->al, d->name, fill)) {
      snprintf (err, errlen, "packing pool %d (%d sequences, the first is %s): %s; %ld sequences were packed before", d->n_pool, fill, d->name[0], d->pk->err, d->pk->kept);
      return -1;
    }
    for (int c = 0; c < fill; c++) {
      d->n_output++;
      if (!d->write_text) continue;
      const char *row = d->aln + (size_t) c * (aln_length + 1);
      if (d->to_screen) printf (">%s\n%s\n", d->name[c], row);
      else write_fasta_record (d->outstream, d->name[c], row);
    }
  }
  if (d->count / 5000 > before / 5000) {
    fprintf (stderr, "%d\t sequences read, %d \t aligned. %.3lf secs elapsed.\n", d->count, d->n_output, biomcmc_update_elapsed_time (d->time1));
    fflush (stderr);
  }
  return 0;
}

/* all files through the route above; whatever ends it, what was aligned so far is closed as a complete file before the command gives up */
static void
align_device_parse (struct align_parse *d, const char **fasta, int n_fasta, size_t block_bytes, int device)
{
  char msg[1024], failed[1024];
  const int max_records = block_bytes / 4 + 1 < PARSE_MAX_RECORDS ? (int) (block_bytes / 4 + 1) : PARSE_MAX_RECORDS;      /* (a record has four bytes at least) */
  if (uvaia_gpu_fasta_open (&d->fasta, device, block_bytes, max_records)) biomcmc_error ("%s", uvaia_gpu_fasta_last_error (NULL));
  d->rec = (uvaia_gpu_fasta_record *) biomcmc_malloc ((size_t) max_records * sizeof (uvaia_gpu_fasta_record));
  d->acgt = (int *) biomcmc_malloc ((size_t) max_records * sizeof (int));
  d->sel = (int *) biomcmc_malloc ((size_t) max_records * sizeof (int));
  d->offsets = (int64_t *) biomcmc_malloc (((size_t) d->pool + 1) * sizeof (int64_t));
  uint64_t bytes = 0;
  for (int j = 0; j < n_fasta; j++) {
    uint64_t nb = 0;
    fprintf (stderr, "Started  reading file %s\n", fasta[j]);
    fasta_blocks fb = fasta_blocks_open (fasta[j], block_bytes, uvaia_gpu_fasta_pinned_alloc, uvaia_gpu_fasta_pinned_free, msg, sizeof msg);
    const int rc = fb ? fasta_blocks_run (fb, max_records, align_parse_scan, d, align_parse_records, d, &nb, msg, sizeof msg) : -1;
    const int broken = fasta_blocks_finish (fb, failed, sizeof failed);      /* a decompressor that failed mid-stream: that is the finding, not what its cut end looked like */
    if (rc || broken) {
      if (d->outstream) biomcmc_close_compress (d->outstream);
      if (d->pk) uvdb_packer_close (d->pk);
      ins_table_close (d->ins);
      var_table_close (d->var);
      if (broken) biomcmc_error ("%s", failed);
      const int text = strstr (msg, "FASTA text:") || strstr (msg, "does not fit a block");     /* what the parser refuses, the line reader takes */
      biomcmc_error ("%s%s", msg, text ? " (--device-parse takes regular FASTA whose records fit a block: `uvaialign` without it reads this file line by line)" : "");
    }
    bytes += nb;
    fprintf (stderr, "Finished reading file %s. In total %d sequences have been read.\n", fasta[j], d->count);
    fflush (stderr);
  }
  double ms[2] = {0., 0.}, ms_seq[2] = {0., 0.};
  uvaia_gpu_fasta_kernel_ms (d->fasta, ms, 0);
  uvaia_gpu_fasta_sequences_ms (d->fasta, ms_seq, 0);
  fprintf (stderr, "device parse: {\"bytes\": %llu, \"block_bytes\": %zu, \"scan_ms\": %.3f, \"count_ms\": %.3f, \"sequences_ms\": %.3f, \"align_ms\": %.3f}\n", (unsigned long long) bytes, block_bytes, ms[0], ms_seq[0],
           ms_seq[1], d->align_ms);
  uvaia_gpu_fasta_close (d->fasta);
  free (d->rec); free (d->acgt); free (d->sel); free (d->offsets);
}

int
main (int argc, char **argv)
{
  int help = 0, version = 0, to_screen = 0, pool = 256 * omp_get_max_threads (), device = 0, errors = 0, n_fasta = 0, compact = 0, device_parse = 0, ch;   /* src/align.c:59-63 */
  size_t parse_block = FASTA_BLOCK_BYTES;
  int devices[64], n_devices = 0;
  double ambig = 0.5, ambig_r = 0.5;
  const char *out = NULL, *ref_file = NULL, *packed = NULL, *insertions = NULL, *variants = NULL, *qc = NULL;
  static const struct option longopts[] = {
    {"help", no_argument, 0, 'h'}, {"version", no_argument, 0, 'v'}, {"stdout", no_argument, 0, 1000}, {"ambiguity", required_argument, 0, 'a'},
    {"pool", required_argument, 0, 'p'}, {"reference", required_argument, 0, 'r'}, {"nthreads", required_argument, 0, 't'},
    {"output", required_argument, 0, 'o'}, {"device", required_argument, 0, 1001}, {"devices", required_argument, 0, 1002},
    {"packed", required_argument, 0, 1003}, {"ref_ambiguity", required_argument, 0, 'A'}, {"compact", no_argument, 0, 1004},
    {"device-parse", no_argument, 0, 1005}, {"parse-block", required_argument, 0, 1006}, {"insertions", required_argument, 0, 1007},
    {"variants", required_argument, 0, 1008}, {"qc", required_argument, 0, 1009},
    {0, 0, 0, 0}};
  while ((ch = getopt_long (argc, argv, "hva:p:r:t:o:A:", longopts, NULL)) != -1) switch (ch) {
    case 'h': help = 1; break;
    case 'v': version = 1; break;
    case 1000: to_screen = 1; break;
    case 'a': ambig = atof (optarg); break;
    case 'p': pool = atoi (optarg); break;
    case 'r': if (ref_file) errors++; ref_file = optarg; break;
    case 't': break;                                  /* the alignments run on the GPU: host threads do not matter */
    case 'o': out = optarg; break;
    case 1001: device = atoi (optarg); break;
    case 1002: n_devices = uvaia_parse_device_list (optarg, devices, 64); if (!n_devices) { fprintf (stderr, "--devices: expected a list such as 0-7 or 0,2,3\n"); exit (EXIT_FAILURE); } break;
    case 1003: packed = optarg; break;
    case 1004: compact = 1; break;
    case 1005: device_parse = 1; break;
    case 1006: parse_block = (size_t) strtoull (optarg, NULL, 10); break;      /* (for tests: the block size of --device-parse in bytes) */
    case 1007: insertions = optarg; break;
    case 1008: variants = optarg; break;
    case 1009: qc = optarg; break;
    case 'A': ambig_r = atof (optarg); break;
    default: errors++;
  }
  const char **fasta = (const char **) argv + optind;
  n_fasta = argc - optind;
  if (version) { printf ("%s\n", UVAIA_PACKAGE_VERSION); return EXIT_SUCCESS; }
  if (!help && !errors && compact && !packed) {
    fprintf (stderr, "--compact chooses the form of the packed database: it needs --packed <out.uvdb>\n");
    errors++;
  }
  if (!help && !errors) {   /* the tables are files of their own: none of them is another table or an output of -o or --packed */
    const char *table[3] = {insertions, variants, qc};
    static const char *const table_opt[3] = {"--insertions", "--variants", "--qc"};
    size_t outlen = 0;
    char *text_out = out ? outfile_from_prefix (out, &outlen) : NULL;
    for (int i = 0; i < 3 && !errors; i++) {
      if (!table[i]) continue;
      for (int k = i + 1; k < 3 && !errors; k++) if (table[k] && !strcmp (table[i], table[k])) {
        fprintf (stderr, "%s and %s name the same file %s: every table needs a file of its own\n", table_opt[i], table_opt[k], table[i]);
        errors++;
      }
      if (!errors && text_out && !to_screen && !strcmp (table[i], text_out)) { fprintf (stderr, "%s names %s, the file -o writes the alignment to\n", table_opt[i], table[i]); errors++; }
      if (!errors && packed && !strcmp (table[i], packed)) { fprintf (stderr, "%s names %s, the database --packed writes\n", table_opt[i], table[i]); errors++; }
    }
    free (text_out);
    if (errors) return EXIT_FAILURE;
  }
  if (help || errors || !ref_file || n_fasta < 1 || pool < 1) {
    printf ("%s \nAlign query sequences against a reference\nThe complete syntax is:\n\n", UVAIA_PACKAGE_STRING);
    printf (" %s [-hv] [--stdout] [-p <int>] [-t <int>] [-o <without suffix>] [-a <double>] [--packed <out.uvdb> [--compact]] [-A <double>] [--device-parse] [--insertions <file>] [--variants <file>] [--qc <file>] -r <ref.fa|ref.fa.xz> <seqs.fa|seqs.fa.xz> [<seqs.fa|seqs.fa.xz>]...\n\n", basename (argv[0]));
    printf ("  -h, --help                       print a longer help and exit\n  -v, --version                    print version and exit\n");
    printf ("  --stdout                         print alignment to stdout (to redirect/pipe) instead of compress to file; much faster but may generate a big output\n");
    printf ("  -p, --pool=<int>                 How many query sequences are read in batch, to be aligned in parallel (defaults to 256 per thread)\n");
    printf ("  -t, --nthreads=<int>             accepted for compatibility (the alignments run on the GPU)\n");
    printf ("  -o, --output=<without suffix>    prefix of xzipped output alignment\n");
    printf ("  -a, --ambiguity=<double>         maximum allowed ambiguity for sequence to be excluded (default=0.5)\n");
    printf ("  -r, --reference=<ref.fa|ref.fa.xz> reference sequence in fasta format, possibly compressed with gz, xz, bz2\n");
    printf ("  <seqs.fa|seqs.fa.xz>             sequences to align in fasta format, possibly compressed with gz, xz, bz2 (can be multiple files)\n");
    printf ("  --device=<int>                   GPU to use (default 0)\n");
    printf ("  --devices=<list>                 several GPUs, e.g. 0-7 or 0,2,3: every pool of queries is cut among them (same rows as one GPU)\n");
    printf ("  --packed=<out.uvdb>              write the aligned sequences straight into a packed database, the file `uvaiapack` makes of the text output;\n");
    printf ("                                   the text itself is then written only if -o or --stdout is given as well (one GPU only)\n");
    printf ("  --compact                        with --packed: write the compact form of the database, the file `uvaiapack --compact` makes of the text output\n");
    printf ("                                   (several times smaller; encoded on the GPU once its base row is fixed, after 4096 sequences)\n");
    printf ("  -A, --ref_ambiguity=<double>     with --packed: maximum allowed ambiguity for an ALIGNED sequence to be kept in the database (default=0.5), as in `uvaiapack`\n");
    printf ("  --device-parse                   split the text into sequences on the GPU instead of reading it line by line, and hand them to the aligner where\n");
    printf ("                                   they lie: the same output, from regular FASTA only (a NUL byte, text before the first header and a header\n");
    printf ("                                   without sequence are refused).  One GPU only; goes with -o, --stdout, --packed and --compact\n");
    printf ("  --insertions=<file>              write the characters the alignment drops -- insertions relative to the reference -- as a table\n");
    printf ("                                   sequence,ref_pos,length,bases: one line per run, ref_pos = reference sites to its left (0 = before the first);\n");
    printf ("                                   compressed by the file's suffix (gz, xz, bz2).  Goes with every other option\n");
    printf ("  --variants=<file>                write what every aligned sequence differs from the reference by as a table sequence,kind,ref_pos,length,ref,alt:\n");
    printf ("                                   S = substitution (a base A C G T unlike the reference; ref and alt), D = deletion (a run of gaps from ref_pos on),\n");
    printf ("                                   I = insertion (ref_pos sites to its left, the bases in alt); by ref_pos within a sequence.  Compressed by suffix\n");
    printf ("  --qc=<file>                      write one line per aligned sequence:\n");
    printf ("                                   sequence,length,score,matches,substitutions,deletions,deleted_sites,insertions,inserted_bases,unknown_sites,other_sites,first_site,last_site\n");
    printf ("                                   (first_site, last_site: the first and last reference site that is no gap).  Both go with every other option\n");
    printf ("  --parse-block=<bytes>            with --device-parse: the text is read in blocks of this size (64 to 1073741824, default 67108864); a record\n");
    printf ("                                   must fit one\n");
    if (help) {
      printf ("Based on the wavefront algorithm (WFA, https://github.com/smarco/WFA), computed on the GPU.\n");
      printf ("Since the sequences are assumed to be similar, sequences too short or too big w.r.t. the reference are rejected.\n\n");
      printf ("The reference sequence and the unaligned fasta files can be compressed with gz, xz, bz2. The alignment output will be compressed with xz, ");
      printf ("unless you miss the tool. In this case the next available compression is tried (then the file extension might not correspond to it).\n\n");
      printf ("The command `pool` is the number of unaligned sequences read into memory at once (the higher the better, given your memory constraints).\n");
    }
    return (help && !errors) ? EXIT_SUCCESS : EXIT_FAILURE;
  }
  if (ambig < 0.001) ambig = 0.001;                   /* src/align.c:132-133 */
  if (ambig > 1.) ambig = 1.;
  if (ambig_r < 0.001) ambig_r = 0.001;               /* pack_main.c:46-47 */
  if (ambig_r > 1.) ambig_r = 1.;
  if (packed && n_devices > 1) {   /* the rows of a pool would lie on several cards and a tile takes 64 consecutive ones: not built */
    fprintf (stderr, "--packed writes the database from the rows on ONE GPU: give --device, or a --devices list of one device (%d were listed)\n", n_devices);
    return EXIT_FAILURE;
  }
  if (device_parse && n_devices > 1) {   /* the parser's buffer, which the aligner loads its pool from, lies on one card */
    fprintf (stderr, "--device-parse hands the sequences to the aligner in the memory of ONE GPU: give --device, or a --devices list of one device (%d were listed)\n", n_devices);
    return EXIT_FAILURE;
  }
  if (device_parse && (parse_block < 64 || parse_block > ((size_t) 1 << 30))) { fprintf (stderr, "--parse-block: expected 64 to 1073741824 bytes\n"); return EXIT_FAILURE; }
  if (!device_parse && parse_block != FASTA_BLOCK_BYTES) { fprintf (stderr, "--parse-block sets the block size of --device-parse: it needs that option\n"); return EXIT_FAILURE; }
  const bool write_text = !packed || out || to_screen;
  int64_t time0[2], time1[2];
  biomcmc_get_time (time0);
  fprintf (stderr, "program: %s package: %s\n", basename (argv[0]), UVAIA_PACKAGE_STRING);

  size_t outlength = 0;
  char *outfilename = NULL;
  if (to_screen) fprintf (stderr, "Sequences will be shown uncompressed in screen (to redirect to file or pipe into another software).\n");
  else if (write_text) {
    char randname[32];
    if (!out) { sprintf (randname, "uvaia.%" PRIx64, (uint64_t) time0[1] & 0xffffff); out = randname; }     /* src/align.c:155-159 */
    outfilename = outfile_from_prefix (out, &outlength);
    fprintf (stderr, "Sequences will be compressed (if possible) and saved into file %s.\n", outfilename);
  }

  /* 1. the reference sequence (src/align.c:163-175): first record of the file */
  readfasta_t rfas = new_readfasta (ref_file);
  if (readfasta_next (rfas) < 1) biomcmc_error ("Error reading reference sequence %s", ref_file);
  char *refseq = rfas->seq; rfas->seq = NULL;
  const size_t aln_length = rfas->seqlength;
  del_readfasta (rfas);
  if (aln_length > 0x3fffffff) biomcmc_error ("reference sequence of %zu sites is too long", aln_length);
  if (compact && aln_length > UVDB_COMPACT_MAX_NCHAR) biomcmc_error ("--compact: alignments of more than %d sites have no compact form (%zu sites)", UVDB_COMPACT_MAX_NCHAR, aln_length);
  /* alignments of different queries do not depend on each other: with several GPUs every pool is cut into contiguous shares, one
     aligner and one host thread per GPU (replicas of src/align.c's per-thread aligners, no exchange) */
  if (!n_devices) { n_devices = 1; devices[0] = device; }
  uvaia_aligner *gpu[64];
  for (int d = 0; d < n_devices; d++) if (uvaia_align_open (&gpu[d], refseq, (int) aln_length, devices[d], NULL)) biomcmc_error ("%s", uvaia_align_last_error (NULL));
  if (n_devices > 1) fprintf (stderr, "Batches of %d sequences will be read and aligned on %d GPUs.\n", pool, n_devices);
  else fprintf (stderr, "Batches of %d sequences will be read and aligned on GPU %d.\n", pool, devices[0]);

  struct uvdb_packer pk;
  double align_ms = 0.;
  if (packed) {
    if (uvdb_packer_open (&pk, packed, (int) aln_length, ambig_r, devices[0], pool, compact)) biomcmc_error ("%s", pk.err);
    fprintf (stderr, "Aligned sequences with at least %d valid sites will be packed into %s.\n", pk.non_n_ref, packed);
  }
  file_compress_t outstream = (to_screen || !write_text) ? NULL : biomcmc_open_compress (outfilename, "w");
  struct ins_table ins;
  ins_table_open (&ins, insertions);
  if (insertions) {
    for (int d = 0; d < n_devices; d++) if (uvaia_align_set_insertions (gpu[d], 1, 0)) biomcmc_error ("%s", uvaia_align_last_error (gpu[d]));
    fprintf (stderr, "Insertions relative to the reference will be saved into file %s.\n", insertions);
  }
  struct var_table var;
  var_table_open (&var, variants, qc);
  if (variants || qc) {   /* the I lines and the insertion counts come from the insertion records */
    for (int d = 0; d < n_devices; d++) if (uvaia_align_set_insertions (gpu[d], 1, 0) || uvaia_align_set_variants (gpu[d], 1)) biomcmc_error ("%s", uvaia_align_last_error (gpu[d]));
    if (variants) fprintf (stderr, "Substitutions, deletions and insertions relative to the reference will be saved into file %s.\n", variants);
    if (qc) fprintf (stderr, "One line of counts per aligned sequence will be saved into file %s.\n", qc);
  }
  char **seq = (char **) biomcmc_malloc ((size_t) pool * sizeof (char *)), **name = (char **) biomcmc_malloc ((size_t) pool * sizeof (char *));
  int *len = (int *) biomcmc_malloc ((size_t) pool * sizeof (int));
  char *aln = write_text ? (char *) biomcmc_malloc ((size_t) pool * (aln_length + 1)) : NULL;
  int count = 0, n_output = 0, n_pool = 0;
  const int print_interval = 5000;
  double result[3];

  biomcmc_get_time (time1);
  if (device_parse) {
    struct align_parse d;
    memset (&d, 0, sizeof d);
    d.al = gpu[0]; d.pk = packed ? &pk : NULL; d.ins = &ins; d.var = &var; d.len = len; d.outstream = outstream; d.to_screen = to_screen; d.write_text = write_text;
    d.aln_length = aln_length; d.ambig = ambig; d.pool = pool; d.name = name; d.aln = aln; d.time1 = time1;
    align_device_parse (&d, fasta, n_fasta, parse_block, devices[0]);
    count = d.count; n_output = d.n_output; align_ms = d.align_ms;
  } else for (int j = 0; j < n_fasta; j++) {
    fprintf (stderr, "Started  reading file %s\n", fasta[j]);
    rfas = new_readfasta (fasta[j]);
    bool end_of_file = false;
    while (!end_of_file) {
      int fill = 0;
      while (fill < pool) {                           /* the serial slot-filling loop with its filters (src/align.c:189-221) */
        if (readfasta_next (rfas) < 0) { end_of_file = true; break; }
        if (!rfas->seq) continue;                     /* a header without sequence lines */
        count++;
        bool seq_valid = true;
        if (((3 * rfas->seqlength) < (2 * aln_length)) || ((2 * rfas->seqlength) > (3 * aln_length))) {
          fprintf (stderr, "Sequence %s has size too different from reference (%lu vs %lu)\n", rfas->name, (unsigned long) rfas->seqlength, (unsigned long) aln_length);
          seq_valid = false;
        }
        if (seq_valid) biomcmc_count_sequence_acgt (rfas->seq, rfas->seqlength, result);
        if (seq_valid && (result[2] > ambig)) {
          fprintf (stderr, "Sequence %s has proportion of N etc. (=%lf) above threshold of %lf\n", rfas->name, result[2], ambig);
          seq_valid = false;
        }
        if (seq_valid && (result[0] < 1. - 1.1 * ambig)) {
          fprintf (stderr, "Sequence %s has proportion of ACGT (=%lf) below threshold of %lf\n", rfas->name, result[0], 1. - 1.1 * ambig);
          seq_valid = false;
        }
        if (!seq_valid) continue;                     /* readfasta_next frees what it still owns */
        seq[fill] = rfas->seq; rfas->seq = NULL;
        name[fill] = rfas->name; rfas->name = NULL;
        len[fill] = (int) rfas->seqlength;
        fill++;
      }
      if (fill) {
        int failed = -1;
        n_pool++;
        if (packed) {   /* one GPU: the steps of uvaia_align_batch, the copy of the text only if somebody reads it */
          double ms = 0.;
          if (uvaia_align_load (gpu[0], (const char *const *) seq, len, fill) || uvaia_align_run (gpu[0]) || (write_text && uvaia_align_fetch (gpu[0], aln, NULL))) failed = 0;
          else if (!uvaia_align_stats (gpu[0], NULL, NULL, NULL, &ms)) align_ms += ms;
        } else {
#pragma omp parallel for num_threads(n_devices) schedule(static, 1)
          for (int d = 0; d < n_devices; d++) {
            const int a = (int) ((long long) fill * d / n_devices), b = (int) ((long long) fill * (d + 1) / n_devices);
            if (b > a && uvaia_align_batch (gpu[d], (const char *const *) seq + a, len + a, b - a, aln + (size_t) a * (aln_length + 1), NULL)) {
#pragma omp critical
              failed = d;
            }
          }
        }
        if (failed >= 0) {   /* what was aligned so far stays a complete file: close the stream before giving up */
          const int a = (int) ((long long) fill * failed / n_devices), b = (int) ((long long) fill * (failed + 1) / n_devices);
          if (outstream) biomcmc_close_compress (outstream);
          if (packed) uvdb_packer_close (&pk);
          ins_table_close (&ins);
          var_table_close (&var);
          biomcmc_error ("%s (counted from sequence %s, the first of the %d handed to device %d; %d sequences were written before)",
                         uvaia_align_last_error (gpu[failed]), name[a], b - a, failed, n_output);
        }
        for (int d = 0; d < n_devices; d++) {   /* the slices of the pool in their order: a record counts its query from the slice's start */
          const int a = (int) ((long long) fill * d / n_devices), b = (int) ((long long) fill * (d + 1) / n_devices);
          if (b > a && ins_table_add (&ins, gpu[d], name + a)) {
            if (outstream) biomcmc_close_compress (outstream);
            if (packed) uvdb_packer_close (&pk);
            ins_table_close (&ins);
            var_table_close (&var);
            biomcmc_error ("%s (insertions of the %d sequences from %s on, handed to device %d; %d sequences were written before)", ins.err, b - a, name[a], d, n_output);
          }
          if (b > a && var_table_add (&var, gpu[d], name + a, len + a)) {
            if (outstream) biomcmc_close_compress (outstream);
            if (packed) uvdb_packer_close (&pk);
            ins_table_close (&ins);
            var_table_close (&var);
            biomcmc_error ("%s (variants of the %d sequences from %s on, handed to device %d; %d sequences were written before)", var.err, b - a, name[a], d, n_output);
          }
        }
        if (packed && packer_add_pool (&pk, gpu[0], name, fill)) {   /* both files stay complete: close them before giving up */
          char msg[640];
          snprintf (msg, sizeof msg, "%s", pk.err);
          if (outstream) biomcmc_close_compress (outstream);
          ins_table_close (&ins);
          var_table_close (&var);
          const long kept = pk.kept;
          uvdb_packer_close (&pk);
          biomcmc_error ("packing pool %d (%d sequences, the first is %s): %s; %ld sequences were packed before", n_pool, fill, name[0], msg, kept);
        }
        for (int c = 0; c < fill; c++) {
          n_output++;
          if (write_text) {
            const char *row = aln + (size_t) c * (aln_length + 1);
            if (to_screen) printf (">%s\n%s\n", name[c], row);
            else write_fasta_record (outstream, name[c], row);
          }
          free (seq[c]); free (name[c]);
        }
      }
      if ((count >= print_interval) && ((count % print_interval) < pool)) {
        fprintf (stderr, "%d\t sequences read, %d \t aligned. %.3lf secs elapsed.\n", count, n_output, biomcmc_update_elapsed_time (time1));
        fflush (stderr);
      }
    }
    del_readfasta (rfas);
    fprintf (stderr, "Finished reading file %s. In total %d sequences have been read.\n", fasta[j], count);
    fflush (stderr);
  }
  if (packed) {
    const long kept = pk.kept, dropped = pk.dropped;
    if (uvdb_packer_close (&pk)) biomcmc_error ("%s", pk.err);
    fprintf (stderr, "Packed %ld of %d aligned sequences (%zu sites) into %s; %ld too ambiguous.\n", kept, n_output, aln_length, packed, dropped);
    fprintf (stderr, "Device time: alignment %.3lf ms; census %.3lf ms, gather %.3lf ms, exception runs %.3lf ms.\n", align_ms, pk.rows_ms[0], pk.rows_ms[1], pk.rows_ms[2]);
    if (compact) fprintf (stderr, "Compact tiles: %ld encoded on the device (count and prefix %.3lf ms, emit %.3lf ms), %ld on the host.\n", pk.tiles_device, pk.encode_ms[0], pk.encode_ms[1], pk.tiles_host);
  }
  if (insertions) {
    fprintf (stderr, "Insertions: %ld sequences with insertions, %lld inserted bases saved to file %s.\n", ins.n_seqs, ins.n_bases, insertions);
    ins_table_close (&ins);
  }
  if (variants || qc) {
    fprintf (stderr, "Variants: %ld sequences with %lld substitutions, %lld deletions (%lld sites) and %lld insertions (%lld bases)", var.n_seqs, var.n_sub, var.n_del, var.n_del_sites, var.n_ins, var.n_ins_bases);
    if (variants) fprintf (stderr, "; records saved to file %s", variants);
    if (qc) fprintf (stderr, "; counts saved to file %s", qc);
    fprintf (stderr, ".\n");
    var_table_close (&var);
  }
  if (to_screen) fprintf (stderr, "Output %d aligned sequences. Total elapsed time: %.3lf secs\n", n_output, biomcmc_update_elapsed_time (time0));
  else if (!write_text) fprintf (stderr, "Aligned %d sequences. Total elapsed time: %.3lf secs\n", n_output, biomcmc_update_elapsed_time (time0));
  else {
    biomcmc_close_compress (outstream);
    fprintf (stderr, "Saved %d sequences to file %s\nTotal elapsed time: %.3lf secs\n", n_output, outfilename, biomcmc_update_elapsed_time (time0));
  }
  for (int d = 0; d < n_devices; d++) uvaia_align_close (gpu[d]);
  free (seq); free (name); free (len); free (aln); free (refseq); free (outfilename);
  return EXIT_SUCCESS;
}
