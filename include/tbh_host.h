/* tbh_host.h — C ABI of libtbh.so: the host-side halves of the write path that the multi-rank command line
 * (tiebrush_amd/ranks.py, `tiebrush --ranks N`) needs outside the `tiebrush` binary.  Plain pointers and sizes; nothing here
 * touches the GPU.
 *
 * Reference interfaces replaced (under /root/reference/src):
 *   tbh_tag_deflate_part   <-  flushPData's tagging of every output record (tiebrush.cpp:506-525, GSam.h:300-305) followed by
 *                              GSamWriter::write -> sam_write1 (GSam.h:648-653), for one rank's slice of the output
 *   tbh_write_bam_parts    <-  the output header the reference builds while it opens its inputs (TInputFiles::addSam,
 *                              tmerge.cpp:57-147: @CO SAMPLE lines, @PG TieBrush) + GSamWriter's open / close (GSam.h:542-580);
 *                              the record stream is the ranks' parts in rank order (BGZF members concatenate)
 * The reference's only multi-worker scheme ends the same way — one collapsed BAM (tiewrap.py:96-126).
 */
#ifndef TBH_HOST_H_
#define TBH_HOST_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TBH_ABI_VERSION 1
int tbh_abi_version(void);
const char* tbh_last_error(void); /* message of the calling thread's last failed call */

/* n output records in output order: record g is the raw BAM record (WITHOUT its block_size field) at blob + rec_off[g],
 * rec_len[g] bytes; yc / yx / yd as tbk_groups_out delivers them.  Tags every record as the reference's flushPData does, frames
 * it, deflates the run into whole BGZF members (no BAM header, no EOF member) on `threads` workers (0: the CPU budget) at
 * `level`, and writes the members to `out_path`.  0 on success, -1 otherwise (tbh_last_error). */
int tbh_tag_deflate_part(const uint8_t* blob, const uint64_t* rec_off, const uint32_t* rec_len, uint32_t n, const double* yc, const int64_t* yx,
                         const int32_t* yd, int level, int threads, const char* out_path);

/* The collapsed BAM of a multi-rank run: the header the single-GPU `tiebrush` writes for the same inputs and command line
 * (version, cmd_argc / cmd_argv = the command line as typed, files in input order), then the members of every part file in
 * the order given, then the EOF member.  The parts are deleted when remove_parts != 0.  0 on success, -1 otherwise. */
int tbh_write_bam_parts(const char* out_path, const char* version, int cmd_argc, const char* const* cmd_argv, int n_files, const char* const* files,
                        int n_parts, const char* const* parts, int remove_parts);

/* 1 when the BAM at `path` was written by TieBrush (a @PG line with PN:TieBrush and a VN tag, tmerge.cpp:70-77), 0 when not,
 * -1 when the header cannot be read. */
int tbh_is_tiebrush(const char* path);

/* The BAM index (BAI, SAM specification 5.2) of the coordinate-sorted BAM at bam_path, by the host builder behind `tiebrush --index`
 * (csrc/host/bai.h; the contract is DESIGN.md 4d), written to bai_path (NULL: bam_path + ".bai").  0 on success, -1 otherwise
 * (tbh_last_error: a reference longer than 2^29 is named). */
int tbh_bai_index_file(const char* bam_path, const char* bai_path);
/* reg2bin of the half-open interval [beg, end) (SAM specification 5.3) */
uint32_t tbh_bai_reg2bin(int64_t beg, int64_t end);

/* The same as a CSI index (CSIv1, min_shift 14), which addresses references beyond 2^29: the builder behind `tiebrush --csi`, written
 * BGZF-compressed to csi_path (NULL: bam_path + ".csi").  0 on success, -1 otherwise. */
int tbh_csi_index_file(const char* bam_path, const char* csi_path);
/* the depth such an index takes for a longest reference of max_len: the smallest d with max_len + 256 <= 2^(14 + 3 d), at most 6 */
int tbh_csi_depth(uint64_t max_len);
/* reg2bin of [beg, end) with `depth` levels below bin 0 (depth 5: tbh_bai_reg2bin); UINT32_MAX for a depth outside [0, 6] or an
 * interval that is empty or not inside [0, 2^(14 + 3 depth)] */
uint32_t tbh_csi_reg2bin(int64_t beg, int64_t end, int depth);

/* The region query behind `tiecov -r` (csrc/host/bai_read.h): the chunks a reader of the 0-based half-open [beg, end)
 * on reference tid has to read, through the index at index_path (NULL: bam_path + ".csi", bam_path + ".bai", then the .bai beside
 * the file's stem, the first that exists; BAI or CSI by its magic).  The chunks are sorted and disjoint: the bins of reg2bins minus
 * the pseudo / meta bin, chunks that end at or before the linear index's (the bin's loff) offset dropped, neighbours that overlap,
 * touch or meet in one BGZF member merged.  Returns the number of chunks; they are written as virtual offsets to chunk_beg /
 * chunk_end when that number is <= cap (otherwise nothing is written: call again with room).  -1 on failure (tbh_last_error): no
 * index, an index whose n_ref is not the header's, a truncated index, tid / beg / end out of range.
 * The reference reads no region and no index (tiecov.cpp walks the whole file): this replaces no interface of it. */
int64_t tbh_index_query(const char* bam_path, const char* index_path, int32_t tid, int64_t beg, int64_t end, uint64_t* chunk_beg, uint64_t* chunk_end,
                        uint64_t cap);

/* ---- Several regions in one run (appended; tbh_abi_version stays 1, the symbols are found by name) ----
 * The region table of `tiecov -R` / `tiebrush -R`: the BED file at bed_path (`chrom start end`, 0-based half-open, tabs or spaces,
 * further columns ignored; blank lines and lines beginning with '#', "track" or "browser" skipped; a trailing CR tolerated) against the
 * header of bam_path, normalised: ends cut to the reference's length, empty intervals dropped, sorted by (tid, beg), intervals that
 * overlap or abut merged.  Returns the number R >= 1 of intervals; they are written to tid / beg / end when R <= cap (otherwise
 * nothing is written: call again with room).  -1 on failure (tbh_last_error names the line): fewer than three fields, a start or end
 * that is not a non-negative integer, start > end, a chrom the header does not list, a file without any region. */
int64_t tbh_regions_from_bed(const char* bam_path, const char* bed_path, int32_t* tid, int64_t* beg, int64_t* end, uint64_t cap);

/* tbh_index_query for a normalised table of n >= 1 intervals (HOST arrays; sorted by (tid, beg), disjoint, non-empty, non-adjacent:
 * anything else is a failure): the union of the intervals' chunk lists, sorted by their begin and merged over the whole set by
 * tbh_index_query's rule, so that no file byte is in two chunks although nearby intervals name the same ones.  For n == 1 the result
 * is tbh_index_query's, element for element.  Return value, cap and failures as there. */
int64_t tbh_index_query_regions(const char* bam_path, const char* index_path, uint32_t n, const int32_t* tid, const int64_t* beg, const int64_t* end,
                                uint64_t* chunk_beg, uint64_t* chunk_end, uint64_t cap);

/* ---- The features of `--features BED --summary OUT` (appended; tbh_abi_version stays 1) ----
 * The BED file at bed_path against the header of bam_path, ONE feature per line in the file's order: nothing is merged, sorted or
 * dropped.  Columns 1-3 as tbh_regions_from_bed reads them (and the same lines skipped), 4 the name (default "."), 5 ignored, 6 the
 * strand '+', '-' or '.' (default '.'); an end beyond the reference is cut to its length.  line[i] is the feature's line in the file,
 * counted from 1.  Returns the number n >= 1 of features; tid / beg / end / strand / line are written when n <= cap, and the names,
 * each closed by a NUL byte, to `names` when they fit names_cap; *names_bytes (optional) = the bytes the names need.  Otherwise nothing
 * of that part is written: call again with room.  -1 on failure (tbh_last_error names the line): what tbh_regions_from_bed refuses, a
 * strand other than + - ., a feature that is empty after the cut, a file without any feature. */
int64_t tbh_features_from_bed(const char* bam_path, const char* bed_path, int32_t* tid, int64_t* beg, int64_t* end, uint8_t* strand, uint64_t* line,
                              uint64_t cap, char* names, uint64_t names_cap, uint64_t* names_bytes);

/* The host summariser behind TBK_SUMMARY_HOST=1 and `tbh_tool summary`: tbk_cov_summary's outputs (include/tbk.h) by plain loops over
 * HOST rows, a feature's products added in row order.  Rows as there: n_intervals interval rows sorted by (tid, start) and disjoint,
 * n_junctions junction rows sorted by (tid, start, end, strand); want_cov / want_junc 0: that part is not computed, its rows are not
 * read and its outputs may be NULL.  strand NULL = all '.'.  Returns 0, or -1 for a null argument or n == 0. */
int tbh_cov_summary_host(uint32_t n, const int32_t* tid, const int64_t* beg, const int64_t* end, const uint8_t* strand, int want_cov, uint32_t n_intervals,
                         const int32_t* iv_tid, const int32_t* iv_start, const int32_t* iv_end, const double* iv_val, int want_junc, uint32_t n_junctions,
                         const int32_t* j_tid, const int32_t* j_start, const int32_t* j_end, const uint8_t* j_strand, const double* j_val,
                         uint64_t* covered, double* sum, double* max, double* junc);

/* The host form of tbk_cov_thresholds behind TBK_SUMMARY_HOST=1 and `tbh_tool depth`: per feature the bases under an
 * interval row (covered [n], may be NULL) and, per threshold, under a row with value >= thr[k] (ge [n][n_thr], feature-major), by a
 * plain loop over HOST rows sorted by (tid, start) and disjoint.  Returns 0, or -1 for a null argument, n == 0, n_thr outside 1 .. 16,
 * a threshold that is NaN, infinite or <= 0, or thresholds that are not strictly ascending. */
int tbh_cov_thresholds_host(uint32_t n, const int32_t* tid, const int64_t* beg, const int64_t* end, uint32_t n_intervals, const int32_t* iv_tid,
                            const int32_t* iv_start, const int32_t* iv_end, const double* iv_val, const double* thr, uint32_t n_thr, uint64_t* covered,
                            uint64_t* ge);
/* `--thresholds LIST` as the command lines parse it: 1 to 16 decimal numbers, finite, > 0, strictly ascending, each parsed completely.
 * Returns their number with thr[0 .. n) filled in (cap >= 16), or -1 with tbh_last_error naming the offending item. */
int tbh_parse_thresholds(const char* list, double* thr, uint32_t cap);

/* ---- The annotation of `--gtf FILE --transcripts OUT` (appended; tbh_abi_version stays 1) ----
 * The GTF file at gtf_path against the header of bam_path: only lines whose third column is `exon` are read (columns 4 and 5 1-based
 * inclusive, 7 the strand, 9 the attributes: transcript_id required, gene_id optional, default "."); transcripts are numbered by the
 * first appearance of their transcript_id, a transcript's exons sorted by start.  Returns the number n_tx >= 1 of transcripts and writes
 * *n_exon; tx_off [n_tx + 1] (CSR into the exon arrays), tid, strand, line (the line of the transcript's first exon line, from 1) are
 * written when n_tx <= tx_cap, ex_beg / ex_end (0-based half-open) when *n_exon <= ex_cap, the names — per transcript its id and its
 * gene, each closed by a NUL byte — when they fit names_cap; *names_bytes (optional) = the bytes they need.  Otherwise nothing of that
 * part is written: call again with room.  -1 on failure (tbh_last_error names the line): an exon line with fewer than nine columns, a
 * coordinate that is not a number, start < 1, end < start, an end beyond the reference, an unknown chrom, a strand other than + - ., no
 * transcript_id, a transcript on two chroms or strands, exons of a transcript that overlap or abut, a file without an exon line. */
int64_t tbh_transcripts_from_gtf(const char* bam_path, const char* gtf_path, uint32_t* tx_off, int32_t* tid, uint8_t* strand, uint64_t* line, uint64_t tx_cap,
                                 int64_t* ex_beg, int64_t* ex_end, uint64_t ex_cap, uint64_t* n_exon, char* names, uint64_t names_cap, uint64_t* names_bytes);

/* The host summariser behind TBK_SUMMARY_HOST=1 and `tbh_tool transcripts`: tbk_tx_summary's outputs (include/tbk.h) by plain loops over
 * HOST rows — tbh_cov_summary_host over the exons and the introns, a transcript's parts added in exon order.  The table and the rows as
 * there; want_cov / want_junc 0: that half is not computed, its rows are not read and its outputs may be NULL.  The four per-exon
 * arrays are optional.  Returns 0, or -1 for a null argument or a table tbk_tx_summary refuses. */
int tbh_tx_summary_host(uint32_t n_tx, uint32_t n_exon, const uint32_t* tx_off, const int32_t* tid, const uint8_t* strand, const int64_t* ex_beg,
                        const int64_t* ex_end, int want_cov, uint32_t n_intervals, const int32_t* iv_tid, const int32_t* iv_start, const int32_t* iv_end,
                        const double* iv_val, int want_junc, uint32_t n_junctions, const int32_t* j_tid, const int32_t* j_start, const int32_t* j_end,
                        const uint8_t* j_strand, const double* j_val, uint64_t* covered, double* sum, double* max, uint32_t* exons_hit, uint32_t* introns_hit,
                        double* junc_min, double* junc_sum, uint64_t* ex_covered, double* ex_sum, double* ex_max, double* in_junc);

/* ---- `--strand-cov PREFIX` (appended; tbh_abi_version stays 1) ----
 * The host form of tbk_cov_split_strand behind TBK_SPLIT_HOST=1: tiecov's input (HOST arrays; flag, yc, yx may be NULL) divided by
 * splice strand by a plain loop.  Class 0 holds the mapped records (flag bit 0x4 clear; flag NULL: all) with strand '+', class 1 '-',
 * class 2 every other byte.  n_rec[3] / n_cig[3] receive the classes' records and CIGAR words.  The output columns hold the classes one
 * after the other, each in the input's order: o_tid, o_pos, o_strand, o_yc, o_yx [n] (class s from n_rec[0] + .. + n_rec[s - 1] on; o_yc /
 * o_yx are written where the input has the column), o_cig [n_cigar_ops] likewise by n_cig, and o_cig_off [n + 3]: class s's n_rec[s] + 1
 * offsets, counted from 0, from element n_rec[0] + .. + n_rec[s - 1] + s on.  Returns 0, or -1 for a null argument. */
int tbh_split_strand_host(uint32_t n, uint32_t n_cigar_ops, const int32_t* tid, const int32_t* pos, const uint16_t* flag, const uint32_t* cig_off,
                          const uint32_t* cig, const double* yc, const uint8_t* strand, const int64_t* yx, uint32_t* n_rec, uint32_t* n_cig, int32_t* o_tid,
                          int32_t* o_pos, uint32_t* o_cig_off, uint32_t* o_cig, double* o_yc, uint8_t* o_strand, int64_t* o_yx);

#ifdef __cplusplus
}
#endif
#endif /* TBH_HOST_H_ */
