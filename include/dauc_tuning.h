/*
 * dauc_tuning.h -- entry points of the TUNING build of the library (tuning/libdauc_tuning.so:
 * the product sources compiled with -DDAUC_TUNING by distributedauc_amd/build.py).
 *
 * These are measured alternatives of the product kernels, kept selectable by number so the
 * measurements behind the product's choices can be repeated (scripts/micro_kernels.py) and so the
 * tests can check that every alternative gives the product's integers. The product library
 * (libdauc.so, include/dauc.h) exports none of them and runs the default of each.
 */
#ifndef DAUC_TUNING_H
#define DAUC_TUNING_H

#include "dauc.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * dauc_surrogate_fwdbwd with an explicit kernel: 0 the product's dispatch, 1 the persistent
 * grid-stride kernel (the small-batch path) at any B, 2 the two-launch form (the streaming kernel
 * writes one fp64 row per workgroup, a second launch reduces them), 3 the streaming kernel alone
 * (dh only: no reduce, no scalar outputs), 20 the product's one-launch kernel (128 extra reducer
 * workgroups, the final one taking the last 512 rows itself) at any unit-stride B, 22 = 20 with its
 * reducers returning at once (the stream and its tagged row stores alone, no scalar outputs: the
 * in-launch hand-off's cost by difference), 23 = 20 with streaming workgroup nblocks / 2 never
 * publishing its row (the reducers' bounded wait times out: NaN outputs and the workspace's status
 * bit, dauc_surrogate_status; seconds of polling -- a test of the timeout path only). The other numbers of rounds 2-3 (round 2's 64 streaming
 * reducers, the early-reducer form, other R / K, stamps; profiles/r03/a) were removed in round 4.
 * Variants 2..23 need unit strides, 16-byte aligned h/dh and int8 labels.
 * Every variant but 23 returns bitwise-identical dh and counts; the fp64 sums agree to rounding.
 */
int dauc_surrogate_fwdbwd_variant(const float* h, int64_t h_stride, const void* y, int y_dtype, int64_t B,
                                  const float* abalpha, const float* p_hat, float* dh, int64_t dh_stride,
                                  double* out64, float* grad3, float* loss, void* workspace,
                                  size_t workspace_bytes, int variant, dauc_stream_t stream);

/*
 * dauc_pd_update_dense with an explicit kernel geometry: variant = v + 4*t, v selects
 * 2 / 1 / 4 / 3 float4 per thread, t = 1 turns the non-temporal loads of g and w0 off, t = 2 makes
 * every load and store non-temporal. Variant 0 is the product's. Results are bit-identical.
 */
int dauc_pd_update_dense_variant(float* w, const float* g, const float* w0, float* w_avg, int64_t n,
                                 float lr, float inv_gamma, int variant, dauc_stream_t stream);

/*
 * dauc_pair_count with an explicit kernel variant: variant = mode + 4*r, mode 0 = packed fp32
 * difference + clamp (exact-compare fallback for tiles with infinities or |score| < 2^-103; the
 * product's), 1 = per-lane VGPR compare counters, 2 = wave ballot + scalar popcount, 3 = mixed;
 * r selects 8 / 4 / 16 positives held per lane. Every variant returns identical counts.
 */
int dauc_pair_count_variant(const float* pos, int64_t P, const float* neg, int64_t N,
                            unsigned long long* wins_ties, int variant, dauc_stream_t stream);

/*
 * Search structure of dauc_auc_counts_sorted_labeled in THIS library (process-wide, default 0).
 * Same integers in every mode.
 *   0: the product's choice -- the count index for tables of up to 219,838 keys, unless the
 *      device finds the table skewed (a cell of 15+ keys, or more than 1.5 keys per cell): then,
 *      and for larger tables, the distinct-key index when the table holds at most 14,000 distinct
 *      keys (tie-heavy tables, round 6), else the LDS search tree;
 *   1: the LDS search tree always (the fallback's structure, tested on every table);
 *   2: the distinct-key index whenever the table holds at most 14,000 distinct keys (the count
 *      index is not built), else the tree -- to test it on any table.
 * Modes 1 and 2 also send dauc_auc_eval_* straight to the sorted path (no count index first).
 */
int dauc_set_search_mode(int mode);

/*
 * Fault injection into the direct count-index build (process-wide, default 0 = none): between the
 * build's count and scatter passes, 1 = one key's cell index past the plan's last cell, 2 = one
 * key moved to the next cell (that cell's counter runs out), 3 = one cell's counter one above its
 * key count. The scatter's index checks must turn each into verdict 2 (the sorted path), never
 * into an out-of-bounds store or wrong counts. Tests only.
 */
int dauc_set_direct_fault(int mode);

/*
 * The count index's build in the exact-AUC evaluations (dauc_auc_eval_counts / _enqueue / _counts_part
 * and the two-step dauc_auc_eval_compact_part / _query_part; process-wide, default 0): 0 the
 * product's cell-slotted build (one count pass inserting every key into its cell's slots, then the
 * query pass, which turns the byte counts into block words itself), 1 round 5's direct build (count,
 * block and scatter passes into the cell-ordered table, then the query; dauc_set_direct_fault acts on
 * it). Same integers; set it before the compaction (which prepares the chosen form's state).
 */
int dauc_set_index_form(int form);

/* The transposing LDS read of the 3x3 weight gradient (csrc/conv_wgrad.hip), for its lane-map test:
 * out[64 lanes][8] <- the 16x16x32 operand fragment (k-step 0, channel block 16) of a [32][64]
 * tile whose element (row, col) holds row * 64 + col. */
int dauc_probe_tr16(short* out, dauc_stream_t stream);

/* The 3x3 weight gradient's form: 0 automatic (stride 1: the window layout of least estimated cost
 * wherever one fits; stride 2: gather), 1 the gather form everywhere, 2 / 3 the window form with
 * per-output-row windows and 64 / 128-pixel chunks, 4 / 5 with shared window rows (stride 1) and
 * 64 / 128-pixel chunks, where they fit (tests, A/B runs). Process-global; tuning builds only. */
int dauc_set_wgrad_form(int form);

/* The launch plan of dauc_bn_act_forward / _backward for an [M, C] activation (csrc/bn_act.hip), from
 * the geometry and constants the launchers use; host arithmetic only, no GPU is touched. For the
 * tests: they derive from it which loops of the kernels a shape runs, so that a retune cannot leave
 * the main loops untested. out[0..11]:
 *   0 TPR, threads per row            1 RPB, rows per pass             2 ctiles, channel tiles
 *   3 nrb, row blocks per tile        4 rows per row block             5 rows per forward group
 *   6 rows per backward group         7 finalize: partial rows per group (subsets x unroll)
 *   8 finalize: row subsets           9 elementwise: vectors per workgroup
 *  10 elementwise: workgroups        11 elementwise: 1 if a thread's channels are hoisted
 * A pass is RPB rows; a group is the passes whose loads the partial-sum kernel issues together (its
 * main loop runs once per whole group of a block's passes, the tail once per remaining pass); the
 * finalize's grouped loop runs when nrb > out[7] - out[8]. DAUC_EINVAL for shapes the kernels refuse. */
#define DAUC_BN_PLAN_WORDS 12
int dauc_bn_launch_plan(int64_t M, int C, int dtype, int64_t out[DAUC_BN_PLAN_WORDS]);

/* The launch plan of dauc_conv3x3_wgrad (csrc/conv_wgrad.hip) for a shape, from the one function the
 * launcher itself launches from, under the form dauc_set_wgrad_form chose; host arithmetic only, no
 * GPU is touched. For the tests: they derive from it which loops of the two kernels a shape runs
 * (a split's chunk loop reaches its steady state from 3 chunks on), so that a retune of the split
 * count or the layouts cannot leave those loops untested. out[0..17]:
 *   0 form: 0 gather, 1 window        1 KT, pixel rows of a chunk's dy tile (gather: 64)
 *   2 shared window rows (0 / 1)      3 R, output rows per chunk       4 KP = R * Wo, its pixels
 *   5 Wd = W + 2, window row width    6 npos, window positions         7 nvec, window vectors per thread
 *   8 images per chunk (0: not shared)                                 9 tiles (grid x)
 *  10 chunks                         11 cps, chunks per split         12 splits (grid y)
 *  13 chunks of the last split       14 output rows (window) / pixels (gather) of the last chunk
 *  15 1 if the grid is placed by XCD (tile_split permutes)            16 LDS bytes of a workgroup
 *  17 KS = KT / 32, k-steps per chunk: the kernel is wgrad3x3_win_kernel<nvec, KS> (gather: 0)
 * Words 2..8 and 17 are 0 in the gather form. DAUC_EINVAL for shapes the launcher refuses. */
#define DAUC_WGRAD_PLAN_WORDS 18
int dauc_conv3x3_wgrad_launch_plan(int64_t N, int H, int W, int Ci, int Ho, int Wo, int Co, int stride,
                                   int64_t out[DAUC_WGRAD_PLAN_WORDS]);

/* The plan of the sorted exact-AUC path (dauc_auc_counts_sorted / _sorted_labeled; csrc/radix_sort.hip,
 * csrc/auc_sort.hip) for a table of M keys (the smaller class), from the functions its launchers
 * launch from (sort_layout, table_plan, dk_tiles); host arithmetic only, no GPU is touched. For the
 * tests: they derive from it which scan form the sort runs, which instantiation of the tree kernels
 * (query_count_kernel<K, .> / query_labeled_kernel<K, .>) counts, and how long the runs of the two
 * one-workgroup scans are, so that a retune of the splitter cap or the tile sizes cannot leave a
 * kernel untested. out[0..15]:
 *   0 sort tiles (2048 keys each)     1 scan form: 0 fused into the scatter, 1 three launches
 *   2 nsum, scan blocks (1024 histogram entries each; launched in form 1 only)
 *   3 block sums per scan_sums_kernel thread (its run loop: >= 2 past 1024 block sums)
 *   4 k, keys per bucket              5 S, splitters = buckets         6 H, tree height
 *   7 stored tree nodes (one padding node per level included)          8 the query's dynamic LDS bytes
 *   9 pad keys written past M (k <= 32: the last bucket is read whole; 0 for larger buckets)
 *  10 K, the kernels' template: k if k <= 32, else 0 (buckets finished by binary searches)
 *  11 distinct-key tiles (1024 keys) 12 tiles per dk_scan_kernel thread
 *  13 kDkMax, the most distinct keys the distinct-key index holds (more: the tree counts)
 *  14 the largest table the count index is built for                  15 kMaxSplit, the cap on S
 * DAUC_EINVAL for M < 1 or M > 0xffffffff (the entry points refuse such tables). */
#define DAUC_SORT_PLAN_WORDS 16
int dauc_sort_table_plan(int64_t M, int64_t out[DAUC_SORT_PLAN_WORDS]);

#ifdef __cplusplus
}
#endif

#endif /* DAUC_TUNING_H */
