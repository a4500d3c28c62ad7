// The exact-AUC evaluation's internal API: what auc_eval.hip (the one-call and two-step
// evaluations) calls in auc_count.hip (the compactions), count_index.hip (the count index built
// straight from the positives), count_query.hip (the query pass through it) and auc_sort.hip (the
// sorted path), and what these units call in one another. Without relocatable device code a kernel
// is launched from the unit that defines it, so the units meet in these host functions.
#pragma once

#include "sort_workspace.h"

namespace dauc {

// The labeled queries of one pass and where their counts go: every score of [begin, end) whose
// label is not 1 is a query; wins_ties[0, 1] += (W, T), *nonfinite (nullable) += the non-finite
// queried scores.
struct LabeledQueries {
    const float* scores;
    const void* labels;
    int label_dtype;
    int64_t begin, end;
    unsigned long long* wins_ties;
    unsigned long long* nonfinite;

    bool valid() const {
        return begin >= 0 && end >= begin && wins_ties != nullptr &&
               (end == begin || (scores != nullptr && labels != nullptr)) && label_dtype_ok(label_dtype);
    }
    bool empty() const { return end == begin; }
};

// auc_count.hip: dauc_compact_positives that also zeroes zero3[0..3) and zero_w[0..nzero_w)
// (used by auc_eval.hip)
int compact_positives_zeroing(const float* scores, const void* labels, int label_dtype, int64_t n, float* pos_out,
                              int64_t* stats, void* workspace, size_t workspace_bytes, unsigned long long* zero3,
                              hipStream_t st, unsigned* zero_w = nullptr, int nzero_w = 0);

// What the compaction's grid does on the side for the stages after it (every pointer nullable):
struct CompactSide {
    unsigned long long* zero3 = nullptr;  // block 0 zeroes zero3[0..3)
    unsigned* zero_w = nullptr;           // the grid zeroes zero_w[0..nzero_w): a later build's per-cell counters
    int nzero_w = 0;
    unsigned long long* put = nullptr;    // block 0: *put = put_val (the two-step slot header's length word)
    unsigned long long put_val = 0ull;
    unsigned* fill_w = nullptr;           // the grid fills nfill16 16-byte words here with all-ones (the slotted
    int64_t nfill16 = 0;                  // table's +inf keys), by extra workgroups past the tiles
};

// auc_count.hip: the evaluations' single-pass, unordered positive compaction. stats[0] (P),
// stats[1], stats[2] (non-finite positives), stats[3] (labels outside {-1, 1}) must be zero on
// entry (a non-zero stats[1]: no tile reserves or writes anything); block 0 zeroes
// zero_next[0..4). At most `cap` positives are stored (stats[0] still counts them all). hist_out
// (required; kCiTop words, zero on entry) += the top-bucket histogram of the positives' keys
// (count_index.h), so a build from them can skip its histogram pass.
int compact_unordered(const float* scores, const void* labels, int label_dtype, int64_t n, float* pos_out, int64_t cap,
                      unsigned long long* stats, unsigned long long* zero_next, unsigned* hist_out,
                      const CompactSide& side, hipStream_t st);

// count_index.hip: the count index built straight from the unsorted positives (no radix sort, no
// tree) and the labeled query pass over scores [begin, end); the table is ordered by cell only.
// The table size M is read from the device (*Mp, the compaction's count), so nothing waits for the
// host; the workspace is carved for Mcap = direct_capacity(n) keys. Without a ready histogram
// the build's own `hist` (kCiTop words at direct_hist_offset(Mcap)) must be zero on entry; with
// one (the table's top-bucket histogram, whose total is the table size), the per-cell counters
// (direct_cnt_ptr) must be. *verdict (device) = 1 when the count index held the table, 2 when the
// caller must run the sorted path (M > Mcap, or a skewed table).
bool direct_enabled();  // the search mode is automatic (always, except in a tuning build's mode 1 / 2)
int64_t direct_capacity(int64_t n);
int64_t direct_hist_offset(int64_t Mcap);  // byte offset of `hist` in the sort workspace
// the per-cell counters the count pass adds into (zeroed by the histogram pass, or by the caller
// when it hands over a ready histogram)
unsigned* direct_cnt_ptr(void* workspace, int64_t Mcap);
int64_t direct_cnt_words();
struct DirectIndex;  // count_index.h
// the direct build alone (4 launches; 3 with a ready histogram: `ready_hist` (kCiTop words, or
// nullptr) already holds the table's top-bucket histogram and the per-cell counters are zero):
// fills *ix with the index's device pointers
int build_direct_index(const float* pos, const unsigned long long* Mp, int64_t Mcap, void* workspace,
                       size_t workspace_bytes, hipStream_t st, DirectIndex* ix, const unsigned* ready_hist = nullptr);
// check (nullable, one u32; the two-step evaluation's consistency word): += #queried scores
// (labels != 1) over [begin, end), mod 2^32 -- counted by the query pass whether or not the index
// held the table.
int counts_labeled_direct(const float* pos, const unsigned long long* Mp, int64_t Mcap, const LabeledQueries& q,
                          unsigned* verdict, void* workspace, size_t workspace_bytes, hipStream_t st,
                          const unsigned* ready_hist = nullptr, unsigned* check = nullptr);

// the two-step evaluation's build + query straight from the gathered slots (no gather copy):
// the count pass reads the slots in place (and writes the part's record header, count_index.h
// SlotSource), then blocks, scatter and the labeled query over [begin, end) as above. The per-cell
// counters must be zero on entry (dauc_auc_eval_compact_part zeroes them; a build leaves them
// zero again).
struct SlotSource;
int counts_labeled_direct_slots(const SlotSource& src, float* pos, int64_t Mcap, const LabeledQueries& q,
                                unsigned* verdict, void* workspace, size_t workspace_bytes, hipStream_t st,
                                unsigned* check);

// the cell-slotted form of the same (round 6; the two-step evaluation's default): one count pass
// inserts every key into its cell's 8-word slot of `stab` (filled with +inf, and the packed byte
// counters and meta's skew word zeroed, by the compaction of step 1), then the query pass, which
// builds the block words from the byte counts itself: two launches instead of four.
int64_t slotted_cells(int64_t Mcap);
size_t slotted_table_bytes(int64_t Mcap);   // primary + secondary + tertiary regions (count_index.h)
size_t slotted_fill_bytes(int64_t Mcap);    // the +inf part: primary + secondary
int64_t slotted_cnt_words();                // the packed byte counters (words) the compaction zeroes
unsigned* slotted_meta_ptr(void* workspace, int64_t Mcap);
// the one-call evaluation's slotted form: the same insertion from the compacted positives `pos`
// (P on the device at *Mp, the top-bucket histogram ready), then the query pass (two launches
// instead of three after the compaction)
int counts_labeled_direct_slotted(const float* pos, const unsigned long long* Mp, int64_t Mcap, unsigned* stab,
                                  const LabeledQueries& q, unsigned* verdict, void* workspace, size_t workspace_bytes,
                                  hipStream_t st, const unsigned* ready_hist);
int counts_labeled_slotted(const SlotSource& src, unsigned* stab, int64_t Mcap, const LabeledQueries& q,
                           unsigned* verdict, void* workspace, size_t workspace_bytes, hipStream_t st,
                           unsigned* check);
// dauc_auc_counts_sorted_labeled with the count index optional: the evaluation's sorted path runs
// only after the count index refused the table (verdict 2), and the sorted table has the same keys
// and the same plan, so it skips that build (count_index = false) and goes to the distinct-key
// index or the tree at once
int counts_sorted_labeled(const float* pos, int64_t P, const LabeledQueries& q, void* workspace,
                          size_t workspace_bytes, hipStream_t st, bool count_index);

// count_query.hip: the labeled query pass through the count index. The form says which build the
// index came from, and with it which query_ci_kernel instantiation runs:
//   sorted            behind a sort (`table` sorted, M on the host): every field null
//   direct            round 5's direct build: the groups' totals, M on the device, the optional check word
//   slotted one-call  the slotted table, the cells' byte counts; no check word
//   slotted two-step  the same with the check word and the grouped end-of-kernel reduction (red8)
struct CiForm {
    unsigned* verdict = nullptr;
    const unsigned* grp = nullptr;
    const unsigned long long* Mp = nullptr;
    unsigned* check = nullptr;
    const uint2* slot_counts = nullptr;
    unsigned slot_cells = 0u;
    unsigned long long* red8 = nullptr;

    static CiForm sorted() { return CiForm{}; }
    static CiForm direct(unsigned* verdict, const unsigned* grp, const unsigned long long* Mp, unsigned* check) {
        CiForm f;
        f.verdict = verdict, f.grp = grp, f.Mp = Mp, f.check = check;
        return f;
    }
    static CiForm slotted_one_call(unsigned* verdict, const unsigned long long* Mp, const uint2* slot_counts,
                                   unsigned slot_cells) {
        CiForm f;
        f.verdict = verdict, f.Mp = Mp, f.slot_counts = slot_counts, f.slot_cells = slot_cells;
        return f;
    }
    static CiForm slotted_two_step(unsigned* verdict, const unsigned long long* Mp, unsigned* check,
                                   const uint2* slot_counts, unsigned slot_cells, unsigned long long* red8) {
        CiForm f = slotted_one_call(verdict, Mp, slot_counts, slot_cells);
        f.check = check, f.red8 = red8;
        return f;
    }
};
int launch_ci(const LabeledQueries& q, const CountWs& cw, const unsigned* table, int64_t M, hipStream_t st,
              const CiForm& form);

}  // namespace dauc
