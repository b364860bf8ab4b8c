// pfmscan_ctx.hpp -- the context object behind the C ABI and the helpers every API translation unit
// shares (error reporting, device scratch).  Not installed.
#pragma once
#include <string>
#include <vector>

#include "pfmscan_internal.hpp"
#include "pfmscan_exact.hpp"

struct pfmscan_motif {
    pfmscan_ctx *ctx = nullptr;
    double *d_letters = nullptr;   // [m][8]
    float *d_pairs = nullptr;      // [(m+1)/2][16] two-letter fp32 sums (4-letter alphabets only), see k_letters_pre
    double pair_eps = 0.0;
    double h_pairsum[16 * 16];     // exact two-letter sums (m <= 32, 4-letter alphabets): operand of the integer prefilter
    bool has_pairsum = false;
    mutable pfmscan::CredCache cred_cache;
    double *h_letters = nullptr;   // host copy of the letter table [m][8] (m <= 32): operand of k_letters_cred8's credits
    mutable pfmscan::Cred8Cache cred8_cache;
    mutable pfmscan::PairCred pair_cred;   // k_pair_cred_sum's tables for the last (structure motif, thr_sum) this sequence motif met
    double *d_struct = nullptr;    // [m][7]
    int m = 0;
    int struct_finite = 0;
    double struct_band = 0.0;      // pfmscan_exact.hpp: half-width of the re-score band of thresholded structure compares
};

namespace pfmscan {
struct Uploader;   // pfmscan_upload.hip: pinned staging buffers + the host threads that fill them
}

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};

struct pfmscan_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr;   // H2D of the next chunk while the previous one is scanned (pfmscan_pipeline.hip)
    std::string err;
    pfmscan::Tuning tune;
    int n_cu = 0;
    int64_t hbm = 0;
    char name[128] = {0};
    DevBuf codes2;                              // second code stream of the two-FASTA combined scan (pfmscan_stage_codes2)
    DevBuf codes, profile, out_seq, out_struct, hit_pos, hit_seq, hit_struct, count;
    DevBuf cand_pos, cand_seq, cand_count;      // candidates of the two-phase combined scan
    DevBuf sort_keys_in, sort_keys_out, sort_vals_in, sort_vals_out, sort_temp, sort_seq, sort_struct;   // pfmscan_sort.hip
    DevBuf sort_motif;                          // library scans: motif index per hit
    DevBuf lib_pos, lib_motif, lib_seq, lib_struct, lib_count;   // library scans: sharded hits of the _dev form
    DevBuf db_in, db_out, db_tree, db_part, db_marks, db_tiles, db_flags;   // dot-bracket annotation (pfmscan_dotbracket.hip)
    DevBuf avg_tab, avg_blk, avg_out;           // fragment averaging (pfmscan_average.hip): tables + T, verdicts, host rows
    DevBuf bg_tab, bg_part, bg_blk, bg_sums;    // profile column sums (pfmscan_background.hip): record tables, piece sums, verdicts, record sums
    DevBuf site_tab, site_blk, site_sums, site_counts;   // site profiles (pfmscan_sites.hip): hit / group / record tables, verdict keys, group sums, group counts
    DevBuf rb_part;                             // profile row bound (pfmscan_rowbound.hip): workgroup partials + the result
    DevBuf mut_tab, mut_best, mut_alt, mut_where, mut_key, mut_valt;   // mutagenesis (pfmscan_mutation.hip): a call's tables, staged outputs, event / variant lists
    DevBuf occ_tab, occ_idx, occ_rec, occ_bs, occ_gs, occ_cnt, occ_out;   // occupancy (pfmscan_occupancy.hip): ratio tables, block / group prefixes, record table, block and level-1 sums, window counts, staged outputs
    DevBuf exp_inv, exp_occ, exp_out;           // expected counts (pfmscan_expect.hip): 1 / occupancy per record and motif, the occupancy when the caller takes none, staged outputs
    DevBuf exp_acc;                             // merged expected counts (pfmscan_expect_merge.hip): the long accumulators and verdicts of a staged call
    DevBuf fp_idx, fp_out, fp_ev;               // posterior site map (pfmscan_footprint.hip): tile prefix of the records, staged planes and occupancy, staged events; pfmscan_mutocc.hip uses them the same way
    DevBuf pipe_codes[2], pipe_profile[2];      // chunked host pipeline: double-buffered chunk of the stream
    hipEvent_t pipe_copied[2] = {nullptr, nullptr}, pipe_scanned[2] = {nullptr, nullptr};
    // host ranges known to be read-only mappings of files (pfmscan_upload_source_file): the staged uploader preads them
    struct FileRange {
        const unsigned char *base = nullptr;
        size_t length = 0;
        int fd = -1;
        int64_t offset = 0;
    };
    static constexpr int N_FILE_RANGES = 8;
    FileRange file_ranges[N_FILE_RANGES];
    int file_range_next = 0;
    pfmscan::Uploader *up = nullptr;
    int upload_mode = PFMSCAN_UPLOAD_RUNTIME;
    // staged stream (pfmscan_stage)
    int64_t staged_n = -1;
    int staged_dtype = PFMSCAN_PROFILE_NONE;
    bool staged_codes = false, staged_profile = false, staged_codes2 = false;
    int64_t stage_serial = 0;                   // counts the stagings: what is cached WITH the staged stream carries the serial it was made for
    // row bound of the staged profile (pfmscan_profile_row_bound_staged), valid while row_bound_serial == stage_serial
    double row_bound = 0.0;
    int64_t row_bound_serial = -1;
    // candidate-then-verify: the last full letters pass was selective -> skip the pilot next time
    bool two_phase_hot = false;
    // which route the last pfmscan_hits_pair_sum_* call with a finite thr_sum took (PFMSCAN_PAIR_ROUTE_*)
    int pair_sum_route = 0;
    // pfmscan_place.hip: sets of arrays placed together (PlaceSet *), and a line about the last allocation
    std::vector<void *> place_sets;
    std::vector<void *> place_retired;        // freed sets kept mapped for the next request of the same sizes
    size_t place_va_reserved = 0;             // address space reserved so far (never given back while the context lives)
    std::string place_note;
};

namespace pfmscan {

int fail(pfmscan_ctx *ctx, int code, const std::string &msg);
int fail_hip(pfmscan_ctx *ctx, hipError_t e, const char *what);
int ensure(pfmscan_ctx *ctx, DevBuf &b, size_t bytes);
void release(DevBuf &b);
// pfmscan_api.hip: argument checks + ScanArgs of a scan of DEVICE buffers; launch on a stream (sharded hits -> sorted host
// arrays: pfmscan_hits.hpp)
int check_and_fill(pfmscan_ctx *ctx, const pfmscan_motif *mo, const uint8_t *d_codes, const void *d_profile, int profile_dtype,
                   int64_t n_pos, ScanArgs &a);
int do_launch(pfmscan_ctx *ctx, const ScanArgs &a, void *stream);
// pfmscan_upload.hip: asynchronous host -> device copy on `st`; the source may be reused when it returns
int upload(pfmscan_ctx *ctx, void *d_dst, const void *h_src, size_t bytes, hipStream_t st);
void upload_release(pfmscan_ctx *ctx);
void place_release_all(pfmscan_ctx *ctx);   // pfmscan_place.hip
// pfmscan_dotbracket.hip: dot-bracket codes d_in -> structure-letter codes d_out on `st` (see pfmscan_dotbracket_annotate_dev)
int dotbracket_annotate(pfmscan_ctx *ctx, const uint8_t *d_in, uint8_t *d_out, int64_t n, const uint8_t *map,
                        int64_t *d_counts, int64_t *host_counts, int64_t *first_bad, hipStream_t st);
// pfmscan_rowbound.hip: the row bound of the staged stream (staged_n > 0 with a profile), measured once per staging.  Synchronises ctx->stream.
int staged_row_bound(pfmscan_ctx *ctx, double *row_sum_max);
inline bool misaligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }

}  // namespace pfmscan

#define HIP_TRY(ctx, expr)                                                  \
    do {                                                                    \
        hipError_t e__ = (expr);                                            \
        if (e__ != hipSuccess) return pfmscan::fail_hip((ctx), e__, #expr); \
    } while (0)
