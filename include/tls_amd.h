/*
 * tls_amd.h -- C ABI of the MI355X transit-least-squares search engine (libtls_amd.so).
 *
 * The reference (hippke/tls v1.0.31) has no FFI layer: its seam for this path is the
 * Python function
 *     search_period(period, t, y, dy, transit_depth_min, R_star_min, R_star_max,
 *                   M_star_min, M_star_max, lc_arr, lc_cache_overview, T0_fit_margin)
 *         -> [period, chi2, row, depth]                 (transitleastsquares/core.py:96-188)
 * mapped over all trial periods by power()              (transitleastsquares/main.py:140-185)
 * and re-sorted by period                               (transitleastsquares/main.py:190-196).
 * This library replaces exactly that: ONE batched call searches every period of one
 * light curve on the GPU and returns chi2/row/depth per period in the order of `periods`.
 * INTEGRATION.md shows the ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - plain C types; every array is contiguous float64 / int64, owned by the caller;
 *     the library copies host->device->host internally and keeps no caller pointer.
 *   - every function returning int returns TLS_OK (0) or a negative TLS_E_* code; the
 *     message is available from tls_last_error(ctx) (ctx may be NULL for create errors).
 *   - a tls_ctx is bound to one GPU and one HIP stream; it is not re-entrant.  Use one
 *     context per GPU (one process per GPU in multi-GPU runs).
 *   - there is NO CPU fallback: without a usable GPU tls_ctx_create fails.
 */
#ifndef TLS_AMD_H
#define TLS_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever a struct of this header changes its layout or an entry point its signature (3: tls_counters has
 * five fields, tls_period_costs / tls_power_batch exist; 4: tls_options, tls_get_options / tls_set_options; 5: tls_options
 * keeps the two caller-facing switches, the developer switches moved behind tls_debug_set_switch, tls_period_costs takes
 * them as text; 6: tls_transit_stats, tls_power_batch_stats, tls_debug_transit_stats; 7: tls_power_batch_models,
 * tls_debug_transit_models).  A binding compares it with tls_abi_version().  Entries added without changing a layout or
 * signature keep the version (7: tls_inject_transits, tls_null_rows, tls_debug_null_words,
 * tls_medfilt_detrend, tls_biweight_detrend), (7: tls_power_batch_peaks, tls_find_peaks),
 * (7: tls_power_batch_peak_fits, tls_debug_peak_fits), (7: tls_phase_scan, tls_power_batch_phase_scan,
 * tls_debug_peak_phase_scans), (7: tls_sysrem), (7: tls_single_transits), (7: tls_transit_times),
 * (7: tls_shape_fit), (7: tls_nudft, tls_lomb_scargle, tls_sine_test); 8: every entry that takes `root, n_root` takes a
 * second table, `root, root_count, n_root`), (8: tls_ephemeris_match), (8: tls_folded_views),
 * (8: tls_event_vetting), (8: tls_centroid_test), (8: tls_noise_profile), (8: tls_transit_fit), (8: tls_remove_transits),
 * (8: tls_event_periods), (8: tls_decorrelate), (8: tls_spline_detrend), (8: tls_clean_rows). */
#define TLS_AMD_ABI_VERSION 8

#define TLS_OK 0
#define TLS_E_ARG (-1)      /* invalid argument */
#define TLS_E_HIP (-2)      /* HIP runtime error (message has the HIP error string) */
#define TLS_E_NOMEM (-3)    /* host or device allocation failed */
#define TLS_E_STATE (-4)    /* call order violated (e.g. execute before prepare) */
#define TLS_E_RCCL (-5)     /* RCCL error */

typedef struct tls_ctx tls_ctx;

/* Optional work counters of one search (all per light curve). */
typedef struct tls_counters {
    int64_t grid_cells;      /* (period, duration, T0) cells enumerated: data independent */
    int64_t evaluated_cells; /* cells that passed mean > transit_depth_min (core.py:58) */
    int64_t inner_steps;     /* template samples multiplied (core.py:67-69) */
    int64_t pd_pairs;        /* (period, duration) pairs searched */
    int64_t issued_fma;      /* lane-FMAs the chi^2 phase issued for them (chunk padding, idle lanes
                                and unroll slack included): inner_steps / issued_fma = lane efficiency */
} tls_counters;

/* Template table = the reference's (lc_cache_overview, lc_arr) of transit.py:98-160,
 * flattened: row r is values[offset[r] .. offset[r]+length[r]), trial width width[r]
 * samples, depth-normalisation factor overshoot[r].
 * 1 <= length[r] <= width[r].  A row SHORTER than its width (an eccentric orbit's table: transit.py:143-149 trims the slow
 * side of the transit) is searched as the reference searches it (core.py:59-70): the window of width[r] samples leaves
 * the out-of-transit sum, the model covers its first length[r] samples, the others count for nothing --
 * chi2 = S0 + rs^2 A - 2 rs B - sum_{j >= length} e_j^2 w_j, with A, B and inner_steps over length[r] taps.  A table with
 * such a row takes the plain classic kernel (LDS-resident series) or the slab kernels: never the four-slot kernel nor the
 * classic kernel's fp32-screen and pruning variants, whatever the switches say (tls_last_kernel reports the choice). */
typedef struct tls_template {
    const double *values;
    const int64_t *offset;
    const int64_t *length;
    const int64_t *width;
    const double *overshoot;
    int64_t n_rows;
} tls_template;

/* Scalar parameters of search_period (core.py:96-109). */
typedef struct tls_params {
    double transit_depth_min;
    double R_star_min, R_star_max, M_star_min, M_star_max;
    double T0_fit_margin;
} tls_params;

/* Switches of a context a caller may set: -1 = the library decides.  They are part of what a prepared plan is keyed by
 * (tls_prepare plans again when they change).  Neither changes a result beyond the distance between the two prefix-sum
 * modes that DESIGN.md section 3 describes (1e-10 relative on chi^2 for a normalised flux; it scales with
 * max|flux| (N + W) 2^-53 / transit depth otherwise).  The developer / test switches that select kernel variants and
 * launch shapes for A/B runs are NOT part of this struct: tls_debug_set_switch below. */
typedef struct tls_options {
    int32_t exact_prefix;   /* 1: every period in exact prefix-sum mode (X = k - numpy.cumsum, bit for bit) */
    int32_t slim;           /* 0: never the four-slots-per-CU kernel of short LDS-resident series (the classic kernel instead) */
} tls_options;

/* ---- context ------------------------------------------------------------------- */
int tls_device_count(void);                 /* number of visible GPUs, <0 on error */
tls_ctx *tls_ctx_create(int device_id);     /* NULL on failure, see tls_last_error(NULL) */
void tls_ctx_destroy(tls_ctx *ctx);
const char *tls_last_error(const tls_ctx *ctx);
const char *tls_version(void);
int tls_abi_version(void);                  /* TLS_AMD_ABI_VERSION the library was built with */
/* "gfx950 ..." style description of the context's device (valid until ctx destroy) */
const char *tls_device_name(const tls_ctx *ctx);
/* the context's switches (see tls_options); tls_set_options drops a prepared plan (the next tls_prepare plans again) */
int tls_get_options(const tls_ctx *ctx, tls_options *out);
int tls_set_options(tls_ctx *ctx, const tls_options *opt);
/* Developer / test switches, by name (not part of the stable ABI; negative value = the library decides): exact_prefix, slim
 * (the two of tls_options), prune, screen32, no_screen (kernel variant of an LDS-resident series), fast_slab, x_staged,
 * sort2, split, split_batch (series in the HBM slab: prefix-sum mode, sort, two-role kernel), threads, blocks, plan_threads
 * (launch shape, host planning), t0_rot (0: the final T0 fit checks every pair of every epoch), prune_min_live, band_max,
 * perm_table (the four-slot kernel's per-plan table of folded orders: 0 none, k > 0 at most k MiB), reg_scan, dense_hoist (its row
 * layout and its fast-mode dense predicate: 0 the former forms), claim_ahead (the tickets of its period queue: bit 0 a
 * workgroup's first ticket is its index; 0 every ticket is drawn from the queue word).  A context starts with the values
 * of the TLS_<NAME> environment variables, read once per process; no call reads the environment after that.
 * One more name, `lanes`, is no planning switch (no part of a plan's key, of tls_debug_get_switches' text or of the
 * environment): 0 sends every search launch to lane A, one after the other on one stream; default on -- back-to-back
 * tls_execute calls of a filled four-slot plan alternate between two launch lanes.  It changes where
 * a launch runs, never a result.
 * tls_debug_get_switches writes all of them as "name=value,name=value" (ctx NULL: the process's) -- the text
 * tls_period_costs takes, so that the planning call prices the kernel the searching context will run. */
int tls_debug_set_switch(tls_ctx *ctx, const char *name, double value);
int tls_debug_get_switches(const tls_ctx *ctx, char *out, int64_t capacity);

/* ---- one-shot search: replaces main.py:140-196 for one light curve -------------- */
/* out_chi2/out_row/out_depth have n_periods entries, index i belongs to periods[i].
 * counters may be NULL. */
int tls_search(tls_ctx *ctx, const double *t, const double *y, const double *dy, int64_t n,
               const double *periods, int64_t n_periods, const tls_template *tmpl,
               const tls_params *params, double *out_chi2, int64_t *out_row,
               double *out_depth, tls_counters *counters);

/* ---- survey mode: many light curves on the SAME time stamps, grids and template ---- */
/* y and dy hold n_curves rows of n values (row-major); the outputs n_curves rows of n_periods.
 * The plan is prepared once (tls_prepare with the first curve) and every further curve only
 * replaces the flux and weights (tls_update_flux), exactly as the staged calls below would.
 * All curves must have the same weight structure (all uniform dy or all per-point dy).
 * Replaces one main.py:140-196 pass per light curve (BASELINE config 5). */
int tls_search_batch(tls_ctx *ctx, const double *t, const double *y, const double *dy, int64_t n,
                     int64_t n_curves, const double *periods, int64_t n_periods,
                     const tls_template *tmpl, const tls_params *params, double *out_chi2,
                     int64_t *out_row, double *out_depth);

/* ---- staged search: same result, inputs resident in HBM between the stages ------ */
/* prepare: validate, build the device-side work list, upload everything (one pinned staging buffer, one
 * asynchronous copy; the call does not wait for the device).  A call with the same t, periods, template and
 * parameters as the plan the context already holds (compared byte for byte) only replaces the flux: that is
 * what a survey and repeated power() calls do, and it costs two passes over y and one upload. */
int tls_prepare(tls_ctx *ctx, const double *t, const double *y, const double *dy, int64_t n,
                const double *periods, int64_t n_periods, const tls_template *tmpl,
                const tls_params *params);
/* replace only the light-curve values of a prepared search (same t, n, grids, template):
 * survey mode streams many light curves through one prepared plan. */
int tls_update_flux(tls_ctx *ctx, const double *y, const double *dy);
/* execute: enqueue the search kernels on the context's stream (asynchronous).
 * count_work & 1 also accumulates evaluated_cells/inner_steps (slower: a kernel instantiation of its own keeps
 * the counters -- the plain one does not carry them --, and counting means evaluating every cell that passes
 * the depth predicate, so the pruning kernel variant is not used). */
int tls_execute(tls_ctx *ctx, int count_work);
/* developer instrumentation: tls_execute(ctx, 2) makes thread 0 of every workgroup stamp
 * the shader clock at phase boundaries -- in the instrumented and the checked library (make clocks / make debug;
 * the shipped library compiles the clock marks out and reports zeros for them, the statistics slots stay);
 * this returns the per-phase cycle sums (up to 26 slots:
 * fold+count, scan, scatter, rank, gather+patch, cumsum, batch prefix, chi2, e-convert,
 * strided predicate, two event counters (cumsum blocks, cumsum fallbacks), tile staging,
 * dense predicate, six cumsum sub-phases, two barrier waits, four pruning steps; names in
 * tls_amd/_lib.py::phase_cycles). */
int tls_debug_phase_cycles(tls_ctx *ctx, uint64_t *cycles, int n);
/* developer/test entry: the kernel's exact parallel evaluation of the sequential fp64 prefix
 * sum (numpy.cumsum order, helpers.py:72) on an arbitrary series of non-negative values;
 * out has count + 1 entries, out[0] = 0. */
int tls_debug_cumsum(tls_ctx *ctx, const double *f, int64_t count, double *out, int threads);
/* developer/test entry: runs the prepared search once more and returns, for every period of the plan, the
 * folded flux y[argsort(phase, stable)] exactly as the kernel's sort left it (core.py:120-123) -- the direct
 * check of the sort order, ties included; out holds n_periods * n doubles (capacity in doubles). */
int tls_debug_folded(tls_ctx *ctx, double *out, int64_t capacity);
/* developer/test entry: likewise the prefix sum C[0..M] of the patched folded flux of every period
 * (helpers.py:72 numpy.cumsum order, core.py:126 patch), M = n + widest window; *row_length = M + 1 (out may be
 * NULL to query it), out holds n_periods * row_length doubles. */
int tls_debug_prefix(tls_ctx *ctx, double *out, int64_t capacity, int64_t *row_length);
/* developer instrumentation: runs the prepared search once more and returns the shader cycles the workgroup that
 * searched period p spent on it (one entry per period of the plan, in `periods` order): the per-period cost the
 * shard cost model of tls_amd/shard.py is fitted to (tools/gpu_cost_model.py). */
int tls_debug_period_cycles(tls_ctx *ctx, uint64_t *cycles, int64_t capacity);
/* developer instrumentation: the debug build (make -C tls_amd/csrc debug) tests every hand-computed
 * bound of the search kernel on the device and counts violations per check (names in
 * tls_amd/_lib.py::check_counts); returns 1 from a checked build, 0 (all counts zero) otherwise. */
int tls_debug_check_counts(tls_ctx *ctx, uint64_t *counts, int n);
/* Test entry: fills the LDS of every CU with `word` (0x7ff80000 pairs read as fp64 NaNs) and, with all-ones bytes, every
 * device buffer of the context that a call fills for itself before it reads it -- the search's per-workgroup scratch (slabs,
 * lists, stashed orders), the post-search chain's arrays, every survey stage's buffer; not the plan, the results, the queues
 * and counters, the batch slots -- on the context's stream: what a previous tenant of the GPU may have left there.  A call
 * after it must return the bits of a call before it (tests/test_gpu_parity.py, tests/test_stage_memory.py: no kernel reads
 * memory it has not written). */
int tls_debug_poison_lds(tls_ctx *ctx, uint32_t word);
/* developer instrumentation: host wall time (ms) of every group of 32 light curves of the context's last tls_power_batch /
 * tls_search_batch call (a stall in one group -- a transfer, a wait, a T0-fit launch -- shows here; bench.py prints the
 * largest and the median).  Returns the number of groups; out may be NULL. */
int tls_debug_batch_group_ms(const tls_ctx *ctx, double *out, int64_t capacity);
/* developer instrumentation: bytes of device memory the context holds, in all (every device buffer it owns) and in the final
 * T0 fit's HBM scratch */
int tls_debug_device_bytes(const tls_ctx *ctx, int64_t *total, int64_t *t0_fit_scratch);
/* developer instrumentation: the table of folded orders of the held plan (four-slot kernel; switch perm_table) -- its size
 * in bytes as the held plan uses it (0: the plan has none; the buffer behind it only grows and is counted by tls_debug_device_bytes) and whether a launch has filled it (1) or the next four-slot launch will (0); plan_reuses
 * (may be NULL): the tls_prepare calls the context has answered from a held plan, which keep the table */
int tls_debug_perm_table(const tls_ctx *ctx, int64_t *bytes, int64_t *filled, int64_t *plan_reuses);
/* developer instrumentation: search launches the context has sent to launch lane A and to launch lane B so far (host-side
 * counters), and whether the lanes are on (switch `lanes`; on may be NULL) */
int tls_debug_lanes(const tls_ctx *ctx, int64_t *lane_a, int64_t *lane_b, int64_t *on);
/* developer instrumentation: what tls_kernel_timing charges each launch it holds (ms, oldest slot of its ring of 64 first):
 * a launch's own event pair, or for an overlapped launch the shorter of that and the time from the end of the launch before
 * it to its own end.  Waits for both lanes.  Returns the number of launches (negative: an error); out may be NULL. */
int tls_debug_launch_ms(tls_ctx *ctx, double *out, int64_t capacity);
/* Test entry: the raw Philox words tls_null_rows draws for trials first_trial .. first_trial + n_rows - 1 with the same
 * (n, seed, mode, block): out [n_rows][W], W = the mode's words per trial rounded up to a multiple of 4 (the last W - words
 * of a row are drawn but not used).  The arguments are checked as tls_null_rows checks them. */
int tls_debug_null_words(tls_ctx *ctx, int64_t n, int64_t n_rows, uint64_t seed, int64_t first_trial, int mode,
                         int64_t block, uint64_t *out);
/* Test entry, host only (no context, no GPU): how the per-candidate stages (tls_transit_times, tls_event_vetting,
 * tls_shape_fit, tls_centroid_test, tls_folded_views, tls_sine_test) cut n_fits candidates into slabs of at most max_fits
 * candidates on at most max_curves distinct curves.  curve [n_fits] (NULL: candidate f reads curve f); out_slab, out_slot
 * [n_fits]: every candidate's slab and the slot of its curve in it; out_runs [n_fits, *n_slabs used]: the row copies a
 * slab takes, consecutive curves in consecutive slots being one; *n_slabs: the slabs there are. */
int tls_debug_candidate_slabs(const int64_t *curve, int64_t n_fits, int64_t max_curves, int64_t max_fits, int64_t *out_slab,
                              int64_t *out_slot, int64_t *out_runs, int64_t *n_slabs);
/* block until the stream is idle */
int tls_synchronize(tls_ctx *ctx);
/* fetch: copy results (and counters, may be NULL) back; synchronises. */
int tls_fetch(tls_ctx *ctx, double *out_chi2, int64_t *out_row, double *out_depth,
              tls_counters *counters);
/* run `reps` executes back to back and report the mean duration of ONE execute in
 * milliseconds, measured with HIP events on the context's stream. */
int tls_execute_timed(tls_ctx *ctx, int reps, double *ms_per_execute);
/* Sum of the search-kernel durations of all executes since the last reset, from HIP
 * events recorded around each launch on the context's stream; synchronises.  The events live in
 * a ring of 64 pairs: with more launches since the last reset, the most recent 64 are summed and
 * *launches says how many that was. */
int tls_kernel_timing(tls_ctx *ctx, int reset, double *total_ms, int64_t *launches);
/* data-independent work of the prepared search (no device work needed). */
int tls_plan_info(const tls_ctx *ctx, tls_counters *counters, int64_t *lds_bytes,
                  int64_t *n_blocks, int64_t *resident /* 1: folded series kept in LDS */);
/* Which search kernel the context's last tls_execute launched: "resident" (LDS-resident series, two or one workgroups
 * per CU), "resident+prune", "resident+screen32", "slim" (LDS-resident, four 256-thread workgroups per CU), "slim512"
 * (the same kernel as two 512-thread workgroups per CU: series of 5121-8889 points with the default duration grid at
 * 30-minute cadence -- beyond the 5120 points of the 256-thread shape, while one region fits half the LDS; the edges move with
 * the duration grid), "slab", "slab+split"; "" before the first launch.  The string is static. */
const char *tls_last_kernel(const tls_ctx *ctx);

/* ---- final T0 fit: the batched counterpart of stats.py:135-204 ------------------------ */
/* For every trial epoch: fold (t, y) at (period, epoch), stable sort by phase, roll the folded
 * flux by `roll` cadences, and return the chi^2 of `signal` (the template row already scaled to
 * the fitted depth, `dur` samples) over the first `dur` samples plus the out-of-transit
 * residuals, both weighted by 1/flux^2 of the twice-rolled flux (the reference's own weighting,
 * stats.py:183-195).  The caller takes the FIRST minimum of out_residuals (stats.py:199-201). */
int tls_t0_fit(tls_ctx *ctx, const double *t, const double *y, int64_t n, double period,
               const double *signal, int64_t dur, const double *epochs, int64_t n_epochs,
               int64_t roll, double *out_residuals);

/* ---- pink noise of the out-of-transit flux: the counterpart of stats.py:72-77 (pink_noise) ---- */
/* mean over all n - width + 1 windows of `width` consecutive points of numpy.std(window) / width ** 0.5, with the reference's
 * roundings: every window's two sums in numpy's pairwise association, the running total added window by window from the left.
 * `root_width` = width ** 0.5 as the caller's language forms it (Python's float power; sqrt(width) otherwise).  data finite;
 * 1 <= width <= n.  (Called per power() by the statistics layer: 3 ms of numpy at TESS size.) */
int tls_pink_noise(tls_ctx *ctx, const double *data, int64_t n, int64_t width, double root_width, double *out);

/* ---- SDE spectra: the counterpart of stats.py:105-132 (spectra) with helpers.py:93-108 ---- */
/* SR, power_raw (scaled to SDE_raw) and power (running-median detrended, scaled to SDE) for the
 * chi^2 of every period; out_sde[0] = SDE_raw, out_sde[1] = SDE.  chi2 == NULL takes the chi^2 array
 * that is still resident on the device from the last tls_execute / tls_search (n is then ignored);
 * `kernel` = oversampling_factor * SDE_MEDIAN_KERNEL_SIZE as the reference forms it (made odd here,
 * stats.py:114-117). */
int tls_spectra(tls_ctx *ctx, const double *chi2, int64_t n, int64_t kernel, double *out_SR,
                double *out_power_raw, double *out_power, double *out_sde);

/* ---- survey-mode power(): search + spectra + final T0 fit of many light curves, all on the device --------- */
/* What main.py:198-283 derives for ONE light curve from the search results -- SDE and SDE_raw (stats.py:105-132),
 * the period and depth at the peak of the detrended power, the template row at the chi^2 minimum, the mid-transit
 * time of the final T0 fit (stats.py:135-204) -- for every light curve of a batch that shares t, the grids and the
 * template (the contract of tls_search_batch).  80 bytes come back per light curve instead of three arrays of
 * n_periods entries; the per-period arrays (chi2/row/depth together, and the detrended power) on request.
 * `median_kernel` = oversampling_factor * SDE_MEDIAN_KERNEL_SIZE (as tls_spectra). */
typedef struct tls_power_summary {
    double SDE, SDE_raw, chi2_min, period, T0, depth;
    int64_t index_best;    /* numpy.argmin(chi2)  (main.py:198) */
    int64_t index_power;   /* numpy.argmax(power) (main.py:270) */
    int64_t best_row;      /* template row at index_best: lc_cache_overview["duration"][best_row] is the duration */
    int64_t no_fit;        /* 1: max(chi2) == min(chi2), "no transit was fit" (main.py:203): SDE 0, depth 1, period NaN */
} tls_power_summary;
int tls_power_batch(tls_ctx *ctx, const double *t, const double *y, const double *dy, int64_t n,
                    int64_t n_curves, const double *periods, int64_t n_periods,
                    const tls_template *tmpl, const tls_params *params, int64_t median_kernel,
                    tls_power_summary *out_summary,
                    double *out_chi2 /* [n_curves][n_periods] or NULL */, int64_t *out_row /* with out_chi2 */,
                    double *out_depth /* with out_chi2 */, double *out_power /* [n_curves][n_periods] or NULL */,
                    double *out_SR /* [n_curves][n_periods] or NULL */, double *out_power_raw /* likewise */);
/* (ABI 5: out_SR / out_power_raw.  With n_curves = 1 and all arrays this is the device part of the drop-in power() call:
 * search, spectra, pick, the final T0 fit's trial epochs and scaled template formed on the device, all fits of a group in one
 * launch, ONE wait per group of 32 light curves.) */
/* The per-transit vetting statistics of power() (api.py:175-241) for one light curve, every field the results key of the
 * same name (the tuples split into _std fields; duration_days is results.duration, in days).  Counts are doubles: a
 * curve without a fit carries NaN in every field but period_uncertainty, like the results object. */
typedef struct tls_transit_stats {
    double period_uncertainty, duration_days;
    double depth_mean, depth_mean_std, depth_mean_even, depth_mean_even_std, depth_mean_odd, depth_mean_odd_std;
    double snr, odd_even_mismatch;
    double transit_count, distinct_transit_count, empty_transit_count;
    double in_transit_count, after_transit_count, before_transit_count;
} tls_transit_stats;
/* tls_power_batch plus the statistics of every light curve, computed on the device behind the final T0 fit of each group
 * and copied back with the group's summaries (still one wait per group).  row_duration: lc_cache_overview["duration"] of
 * every template row (tmpl->n_rows entries); fill_factor: calculate_fill_factor(t); root and root_count: the two forms of
 * k ** 0.5 that power() takes of a count, k = 0 .. n_root - 1 with n_root > n, each formed by the caller's own Python and
 * numpy -- root[k] = float(k) ** 0.5 (Python's pow: snr, the pink-noise width, depth_mean_std) and root_count[k] =
 * numpy.sum(k) ** 0.5 (the power of a numpy integer scalar, which depth_mean_odd_std and depth_mean_even_std divide by and
 * which is one ulp from the other at some k, a set that depends on the numpy build).  A NULL or too short table is
 * TLS_E_ARG with the outputs untouched.  out_per_transit (NULL: not returned): [n_curves][6][max_epochs] --
 * transit_times, per_transit_count, transit_depths, transit_depths_uncertainties, snr_per_transit, snr_pink_per_transit --
 * NaN past a curve's epochs; out_n_epochs (NULL: not returned): epochs of every curve (0 without a fit).  TLS_E_ARG when t
 * is not non-decreasing, or when a curve has more than max_epochs transit epochs. */
int tls_power_batch_stats(tls_ctx *ctx, const double *t, const double *y, const double *dy, int64_t n,
                          int64_t n_curves, const double *periods, int64_t n_periods,
                          const tls_template *tmpl, const tls_params *params, int64_t median_kernel,
                          tls_power_summary *out_summary, double *out_chi2, int64_t *out_row, double *out_depth,
                          double *out_power, double *out_SR, double *out_power_raw,
                          const double *row_duration, double fill_factor, const double *root, const double *root_count,
                          int64_t n_root,
                          tls_transit_stats *out_stats, int64_t max_epochs, double *out_per_transit,
                          int64_t *out_n_epochs);
/* developer/test entry: the statistics stage of tls_power_batch_stats, the same kernel, on picks the caller supplies for
 * light curves y [n_curves][n] on the prepared plan: period, T0, best_row, depth, no_fit, index_power per curve and the
 * detrended power [n_curves][n_periods].  n_curves in [1, 1024]; the other arguments as tls_power_batch_stats. */
int tls_debug_transit_stats(tls_ctx *ctx, const double *y, int64_t n_curves, const double *period, const double *T0,
                            const int64_t *best_row, const double *depth, const int64_t *no_fit, const int64_t *index_power,
                            const double *power, const double *row_duration, int64_t n_rows, double fill_factor,
                            const double *root, const double *root_count,
                            int64_t n_root, int64_t max_epochs, tls_transit_stats *out_stats,
                            double *out_per_transit, int64_t *out_n_epochs);
/* tls_power_batch_stats plus the arrays power() returns for plotting (api.py:175-203), computed on the device behind the
 * statistics of each group and copied back with them (still one wait per group):
 *   out_folded [n_curves][3][n]: folded_phase, folded_y and the order (indices into t, as doubles) that sorts the phases
 *     fold(t, period, T0 + period / 2) ascending.  The order is the stable one: equal phases by index (power()'s
 *     numpy.argsort leaves their order open; for distinct phases the two agree).  folded_dy is dy gathered by that order.
 *   out_model_folded [n_curves][n]: model_folded_model.
 *   out_lc [n_curves][2][lc_cap]: model_lightcurve_time, then model_lightcurve_model, NaN past out_lc_len[c] entries.
 * curve_t / curve_f: the in-transit slice of the supersampled template curve (template.py:52-53, curve_n >= 2 ascending
 * time stamps); curve_lo / curve_hi: the ends of reference_transit's linspace (t[first], t[-first - 1]); maxw:
 * int(max(durations) * n), not rounded up to even (api.py:140).  Every row of a curve without a fit is NaN, its length 0.
 * TLS_E_ARG as tls_power_batch_stats, when lc_cap is below a curve's model light curve, and where power() itself raises
 * (fewer than two model samples, a squeezed transit wider than its window).  out_per_transit may be NULL. */
int tls_power_batch_models(tls_ctx *ctx, const double *t, const double *y, const double *dy, int64_t n,
                           int64_t n_curves, const double *periods, int64_t n_periods,
                           const tls_template *tmpl, const tls_params *params, int64_t median_kernel,
                           tls_power_summary *out_summary, double *out_chi2, int64_t *out_row, double *out_depth,
                           double *out_power, double *out_SR, double *out_power_raw,
                           const double *row_duration, double fill_factor, const double *root, const double *root_count,
                           int64_t n_root,
                           tls_transit_stats *out_stats, int64_t max_epochs, double *out_per_transit,
                           int64_t *out_n_epochs, const double *curve_t, const double *curve_f, int64_t curve_n,
                           double curve_lo, double curve_hi, double maxw, int64_t lc_cap, double *out_folded,
                           double *out_model_folded, double *out_lc, int64_t *out_lc_len);
/* developer/test entry: the statistics and model stages of tls_power_batch_models on injected picks, as
 * tls_debug_transit_stats; the model arguments as tls_power_batch_models. */
int tls_debug_transit_models(tls_ctx *ctx, const double *y, int64_t n_curves, const double *period, const double *T0,
                             const int64_t *best_row, const double *depth, const int64_t *no_fit, const int64_t *index_power,
                             const double *power, const double *row_duration, int64_t n_rows, double fill_factor,
                             const double *root, const double *root_count,
                             int64_t n_root, int64_t max_epochs, tls_transit_stats *out_stats,
                             double *out_per_transit, int64_t *out_n_epochs, const double *curve_t, const double *curve_f,
                             int64_t curve_n, double curve_lo, double curve_hi, double maxw, int64_t lc_cap,
                             double *out_folded, double *out_model_folded, double *out_lc, int64_t *out_lc_len);
/* developer/test entry: the post-search chain of tls_power_batch -- spectra, pick, trial epochs and scaled template, final
 * T0 fit, first minimum, the same code -- on search results the caller supplies: chi2 / row / depth [n_curves][n_periods]
 * and flux y [n_curves][n] of light curves on the prepared plan (tls_prepare: time stamps, periods, template and
 * T0_fit_margin).  n_curves in [1, 1024], all in one group.  TLS_E_ARG when the row at a curve's chi2 minimum is not the
 * first row of a template duration.  Optional (NULL: not returned): every fit's trial epochs and residuals
 * [n_curves][n] (the first out_n_epochs[c] of a row are set), its number of trial epochs, and whether the rotation path
 * handed it back to the general kernel (1), kept it (0), or did not run (-1). */
int tls_debug_post_search(tls_ctx *ctx, const double *y, int64_t n_curves, const double *chi2, const int64_t *row,
                          const double *depth, int64_t median_kernel, tls_power_summary *out_summary,
                          double *out_epochs, double *out_residuals, int64_t *out_n_epochs, int64_t *out_handed_back);

/* ---- survey-mode injection-recovery: transits injected on the device ---------------------------------------------- */
/* Constants of one injected planet on a circular orbit, formed by the caller as transit_model's _true_anomaly (ecc < 1e-5
 * branch) and projected_separation form them: tp = T0 - period * (pi/2 - omega) / (2 pi), sin_inc = sin(radians(inc)),
 * omega = radians(90); rp = Rp/R*, a = a/R*. */
typedef struct tls_injection {
    double tp, period, rp, a, sin_inc, omega;
} tls_injection;
/* out_flux[k][i] = flux[k or 0][i] * transit_model.light_curve(t[i]) of injection k (quadratic law u1, u2; linear: u2 = 0;
 * uniform: u1 = u2 = 0).  flux_rows: 1 (one base row shared by every injection) or n_inj.  out_in_transit[k] (may be NULL):
 * points with z < 1 + rp, 0 for a planet whose transits all fall into gaps.  A point out of contact keeps its base flux bit
 * for bit.  TLS_E_ARG for n < 1, another flux_rows, a non-finite constant, period <= 0, a <= 0 or rp < 0; n_inj == 0 is a
 * no-op. */
int tls_inject_transits(tls_ctx *ctx, const double *t, int64_t n,
                        const double *flux, int64_t flux_rows,
                        const tls_injection *inj, int64_t n_inj,
                        double u1, double u2,
                        double *out_flux,
                        int64_t *out_in_transit);

/* ---- survey-mode false-alarm calibration: null (noise-only) light curves on the device ----------------------------- */
/* out[r][i] for trials R = first_trial + r (r < n_rows), points i < n.  The random stream is Philox4x64-10 under key
 * (seed, 0), word j at counter (j / 4 + 1, 0, 0, 0) as numpy.random.Philox(key=seed).random_raw() orders it; trial R takes
 * words [R W, R W + words), W = words rounded up to a multiple of 4 (numpy.random.Philox(key=seed, counter=R W / 4)
 * .random_raw(W)), so a row depends on (seed, R) alone, not on how the trials are split into calls.
 * mode 0, white noise (words = 2n): u_a = (w[2i] >> 11) 2^-53, u_b = (w[2i+1] >> 11) 2^-53 (numpy Generator.random()),
 *   out = 1 + sigma[r or 0] sqrt(-2 log(1 - u_a)) cos(2 pi u_b) without contraction; n_sigma 1 or n_rows, every sigma in
 *   (0, 0.1].  src, n_src and block are not read.
 * mode 1, block bootstrap (words = ceil(n / block)): trial R copies source row s = R mod n_src of src [n_src][n]; bootstrap
 *   block b (points b block .. min(n, (b+1) block) - 1) starts at start_b = floor(w[b] (n - block + 1) / 2^64), out[i] =
 *   src[s][start_b + i - b block]: copies only, bit-exact.  block in [1, n], every source value finite and > 0.  sigma and
 *   n_sigma are not read.
 * TLS_E_ARG for n outside [1, 1e8], n_rows < 0, first_trial < 0, another mode, a bad sigma, n_sigma, block, n_src or
 * source value, and for trials whose counters would pass 2^64 - 1; n_rows == 0 is a no-op. */
int tls_null_rows(tls_ctx *ctx, int64_t n, int64_t n_rows, uint64_t seed, int64_t first_trial, int mode,
                  const double *sigma, int64_t n_sigma,
                  const double *src, int64_t n_src, int64_t block,
                  double *out);

/* ---- survey-mode detrending: a median filter on the device ------------------------------------------------------- */
/* The largest kernel size tls_medfilt_detrend takes (tls_amd._lib.MEDFILT_MAX_KERNEL mirrors it). */
#define TLS_MEDFILT_MAX_KERNEL 4095
/* For every row r < n_rows of y [n_rows][n]: out_trend[r] = scipy.signal.medfilt(y[r], kernel) -- the median of the `kernel`
 * SAMPLES centred on each point, the row padded with zeros at both ends (ndimage.rank_filter(y, kernel // 2, size=kernel,
 * mode="constant")) -- and out_flat[r] = y[r] / out_trend[r], one IEEE division per point.  The median is a selection, so
 * both are bit-equal to scipy's.  out_trend may be NULL (not returned).  kernel odd, 1 <= kernel <= n and kernel <=
 * TLS_MEDFILT_MAX_KERNEL: the padding then never reaches the median, so every trend value is > 0.  TLS_E_ARG for n outside
 * [1, 1e8], n_rows < 0, an even kernel, one < 1, > n or > TLS_MEDFILT_MAX_KERNEL, and a NaN, infinite or non-positive y;
 * n_rows == 0 is a no-op. */
int tls_medfilt_detrend(tls_ctx *ctx, const double *y, int64_t n, int64_t n_rows, int64_t kernel,
                        double *out_flat, double *out_trend);

/* ---- survey-mode detrending: a time-windowed biweight on the device ---------------------------------------------- */
/* The most points one window of tls_biweight_detrend may hold (tls_amd._lib.BIWEIGHT_MAX_WINDOW mirrors it), and the
 * estimator's fixed constants: the tuning constant C, the relative tolerance FTOL and the iteration cap (mirrored as
 * BIWEIGHT_C, BIWEIGHT_FTOL, BIWEIGHT_MAX_ITER). */
#define TLS_BIWEIGHT_MAX_WINDOW 4095
#define TLS_BIWEIGHT_C 5.0
#define TLS_BIWEIGHT_FTOL 1e-6
#define TLS_BIWEIGHT_MAX_ITER 50
/* For every row r < n_rows of y [n_rows][n] at the time stamps t [n] (shared by all rows, non-decreasing):
 * out_trend[r][i] = Tukey's biweight location of the window of point i and out_flat[r][i] = y[r][i] / out_trend[r][i],
 * one IEEE division per point.  A new segment starts at every j with t[j] - t[j-1] > break_tolerance (days; INFINITY: never);
 * the window of i is every j of i's segment with fabs(t[j] - t[i]) <= 0.5 * window_length (days), a contiguous range that
 * holds i.  In the window's values v: loc = median(v) (the mean (a + b) / 2 of the two middle values for an even count), then
 * up to TLS_BIWEIGHT_MAX_ITER times: mad = median(|v - loc|), stop if mad == 0; u = (v - loc) / (TLS_BIWEIGHT_C * mad),
 * w = (1 - u * u)^2 where |u| < 1, else 0; new = sum(w * v) / sum(w), both sums sequential in ascending index; stop after
 * loc = new if |new - loc| <= TLS_BIWEIGHT_FTOL * |new|.  Every step is one IEEE double operation without contraction, so
 * the result is bit-equal to a restatement of these lines in numpy; every trend value is > 0 and finite.  out_trend may be
 * NULL (not returned).  TLS_E_ARG for n outside [1, 1e8], n_rows < 0, a non-finite or decreasing t, a window_length that is
 * not finite and > 0, a break_tolerance that is not > 0, a window of more than TLS_BIWEIGHT_MAX_WINDOW points, and a NaN,
 * infinite or non-positive y; n_rows == 0 is a no-op. */
int tls_biweight_detrend(tls_ctx *ctx, const double *t, const double *y, int64_t n, int64_t n_rows,
                         double window_length, double break_tolerance, double *out_flat, double *out_trend);

/* ---- survey-mode detrending with the transits protected: the two-pass flow (search, mask, detrend again, search) -------- */
/* The in-transit flags of a batch: out_mask [n_curves][n], 1 = protected, from n_candidates candidates (curve[k] in
 * [0, n_curves), or curve NULL: candidate k belongs to curve k; period[k], T0[k], duration[k] in days).  Point i of curve c is
 * protected if any candidate k of curve c has
 *     d = t[i] - T0[k];  e = floor(d / period[k] + 0.5);  r = d - e * period[k];  fabs(r) <= 0.5 * (factor * duration[k]),
 * one IEEE double operation a step in this order, no contraction.  A candidate takes part only if its period, T0 and duration
 * are finite, its period > 0 and its duration > 0; any other is skipped silently.  The candidates of a curve may come in any
 * order and number; the host groups them by curve (a stable sort), one thread owns one (curve, point).  t need not be sorted.
 * Needs no plan and leaves a prepared one as it is.  n_curves == 0 is a no-op.  TLS_E_ARG, before any device work, for n
 * outside [1, 1e8], a negative count, a factor that is not finite and > 0, a non-finite t and a curve outside [0, n_curves). */
int tls_transit_mask(tls_ctx *ctx, const double *t, int64_t n, const int64_t *curve, const double *period, const double *T0,
                     const double *duration, int64_t n_candidates, double factor, int64_t n_curves, uint8_t *out_mask);
/* tls_biweight_detrend with the protected points (mask [n_rows][n], != 0) left out of every fit.  The windows [lo_i, hi_i) are
 * exactly those of tls_biweight_detrend -- they depend on t alone, and a protected i keeps its window centred on t[i].  The
 * members of window i are its unprotected j, m_i their number.
 *   m_i >= min(min_points, hi_i - lo_i) (min_points >= 1; a window that holds fewer than min_points points altogether is
 *     fitted when none of them is protected, as tls_biweight_detrend fits it): out_trend[i] = the biweight location of the
 *     members by the loop above (median, MAD, reweighting, both sums in ascending index, over the members only); status 0.
 *   otherwise i is open; a and b = the nearest points of status 0 to the left and right in i's segment:
 *     both: trend = ta + (tb - ta) * ((t[i] - t[a]) / (t[b] - t[a])), operations in this order, ta where t[b] == t[a]; status 1
 *     one: that point's trend; status 1
 *     none (every point of the segment is open): the plain biweight of i's own window, the mask ignored; status 2.
 * out_flat = y / trend.  The trend is always defined, so out_flat is finite and > 0 for every input tls_biweight_detrend
 * accepts.  An all-zero mask gives tls_biweight_detrend's out_flat and out_trend bit for bit; an all-ones row the same values
 * with status 2 everywhere.  out_trend and out_status ([n_rows][n]) may be NULL.  TLS_E_ARG as tls_biweight_detrend, and for
 * min_points < 1. */
int tls_biweight_detrend_masked(tls_ctx *ctx, const double *t, const double *y, const uint8_t *mask, int64_t n, int64_t n_rows,
                                double window_length, double break_tolerance, int64_t min_points, double *out_flat,
                                double *out_trend, uint8_t *out_status);

/* ---- survey-mode detrending: SysRem, the systematics the rows share, fitted across them on the device ------------- */
/* The lanes of a row sum and the rows of a column sum's chunk (both part of the definition below), the most components and
 * the most iterations per component (tls_amd._lib.SYSREM_* mirror them). */
#define TLS_SYSREM_LANES 256
#define TLS_SYSREM_ROW_CHUNK 32
#define TLS_SYSREM_MAX_COMPONENTS 8
#define TLS_SYSREM_MAX_ITER 1000
/* SysRem (Tamuz, Mazeh & Zucker 2005) over the rows of y [n_rows][n] on shared epochs: K = n_components rank-1 terms
 * c_i * a_j (star coefficient times epoch profile) are fitted to the residual matrix by alternating weighted least squares and
 * divided out.  Every step is one IEEE double operation without contraction, and two reduction orders are part of the
 * definition:
 *   rowsum(v[0..n)): lane l of TLS_SYSREM_LANES adds v[l], v[l+256], ... in ascending order, starting from 0.0; the 256
 *     partials are folded by the fixed tree: for s = 128, 64, ..., 1: p[l] = p[l] + p[l+s] for l < s; the result is p[0].
 *   colsum(v[0..n_rows)): chunks of TLS_SYSREM_ROW_CHUNK consecutive rows, each summed in ascending row order from 0.0; the
 *     chunk sums added in ascending chunk order from 0.0.
 * The fit (all y finite and > 0; dy, when given, [n_rows][n] finite and > 0):
 *   m_i = rowsum(y_i) / n;  x_ij = y_ij / m_i - 1.0
 *   with dy: r = dy_ij / m_i; w_ij = 1.0 / (r * r)
 *   without: v_i = rowsum(x_i * x_i) / n; w_ij = v_i > 0 ? 1.0 / v_i : 0.0 (a constant row carries no weight and comes out
 *     as y / m)
 *   for k = 0 .. K-1, from c_i = 1.0 and a_prev_j = 0.0, iterations 1 .. max_iter:
 *     a_j = colsum_i((x_ij * c_i) * w_ij) / colsum_i((c_i * c_i) * w_ij), or 0.0 where the denominator is not > 0
 *     c_i = rowsum_j((x_ij * a_j) * w_ij) / rowsum_j((a_j * a_j) * w_ij), or 0.0 likewise
 *     the component is finished after the iteration in which max_j |a_j - a_prev_j| <= tol * max_j |a_j|; otherwise
 *     a_prev = a and the next iteration runs
 *     after the last iteration: x_ij = x_ij - c_i * a_j, C[i][k] = c_i, A[k][j] = a_j, iters[k] = iterations run
 *   s_ij = 0.0; for k ascending: s_ij = s_ij + C[i][k] * A[k][j]
 *   trend_ij = m_i * (1.0 + s_ij);  flat_ij = y_ij / trend_ij
 * The maxima are exact in any order and everything else has its order fixed, so the result -- out_iters and the stop
 * decision included -- is bit-equal to a restatement of these lines in numpy (tests/sysrem_spec.py).  dy, out_trend, out_c
 * [n_rows][K], out_a [K][n] and out_iters [K] may be NULL.  The whole call is one stream submission: max_iter iterations per
 * component are enqueued, and the launches behind a component's convergence return at once on a device-side flag.
 * TLS_E_ARG, before any device work, for n outside [1, 1e8], n_rows < 2, n_components outside [1, min(
 * TLS_SYSREM_MAX_COMPONENTS, n_rows - 1)], max_iter outside [1, TLS_SYSREM_MAX_ITER], a tol that is negative or not finite
 * (0 is allowed: a component then stops only when a repeats itself exactly), and a NaN, infinite or non-positive y or dy.
 * TLS_E_ARG after the device work where a trend value is not finite and > 0 (the fit can overshoot with wildly unequal dy): the
 * message names the first such (row, point), the outputs are unspecified and the context stays usable. */
int tls_sysrem(tls_ctx *ctx, const double *y, const double *dy, int64_t n, int64_t n_rows,
               int64_t n_components, int64_t max_iter, double tol,
               double *out_flat, double *out_trend, double *out_c, double *out_a, int64_t *out_iters);

/* ---- survey mode: the K harmonic-aware peaks of a periodogram, found on the device -------------------------------- */
/* One peak.  chi2, depth and row are the search's values at the peak's index (NaN / -1 where the call has no source for
 * them); entries past a row's n_peaks hold NaN in the doubles and -1 in the integers. */
typedef struct tls_peak {
    double period, power, chi2, depth;
    int64_t index, row;
} tls_peak;
#define TLS_PEAKS_MAX_K 32
#define TLS_PEAKS_MAX_RATIOS 16
/* The selection on one row power[n] over periods[n] (greedy non-maximum suppression with harmonic ratios; the numpy
 * restatement is tests/peaks_spec.py):
 *   cand[j] = (j == 0 or power[j] > power[j-1]) and (j == n-1 or power[j] >= power[j+1]) and power[j] >= min_power
 *   alive = cand; at most k times, while an index is alive:
 *       j = the lowest index of the largest power among the alive ones (numpy.argmax); take j; P = periods[j]
 *       for r in (1.0,) + ratios:  c = r * P;  w = min_separation * c;
 *           alive[i] = false for every i with fabs(periods[i] - c) <= w
 * A NaN fails every comparison (an index holding one, or next to one, is no candidate); c, w and periods[i] - c are one
 * IEEE double operation each, without contraction; `periods` need not be sorted.  The result is a selection: bit-equal to
 * the restatement.  The alive set is a bit mask in the workgroup's LDS up to 2^20 periods and in device memory beyond.
 * Limits (TLS_E_ARG otherwise): 1 <= k <= TLS_PEAKS_MAX_K; min_separation finite and in [0, 1); 0 <= n_ratios <=
 * TLS_PEAKS_MAX_RATIOS, every ratio finite and > 0; min_power not NaN (-INFINITY: none); 1 <= n_periods <= 2^30.
 *
 * tls_find_peaks: rows the caller holds, power [n_rows][n_periods]; chi2, row and depth each NULL or [n_rows][n_periods];
 * out_peaks [n_rows][k], out_n_peaks [n_rows].  n_rows == 0 is a no-op. */
int tls_find_peaks(tls_ctx *ctx, const double *power, const double *chi2, const int64_t *row, const double *depth,
                   int64_t n_rows, int64_t n_periods, const double *periods, int64_t k, double min_separation,
                   const double *ratios, int64_t n_ratios, double min_power, tls_peak *out_peaks, int64_t *out_n_peaks);
/* tls_power_batch_stats plus the peaks of every light curve's detrended power (the row tls_power_batch picks index_power
 * from), selected on the device behind the pick of each group and copied back with the group's summaries (still one wait
 * per group).  The first peak of a curve with a fit is its summary's index_power; a curve without a fit has no peaks.
 * out_stats == NULL: no statistics are computed and row_duration .. out_n_epochs are not read.  out_peaks [n_curves][k],
 * out_n_peaks [n_curves]. */
int tls_power_batch_peaks(tls_ctx *ctx, const double *t, const double *y, const double *dy, int64_t n,
                          int64_t n_curves, const double *periods, int64_t n_periods,
                          const tls_template *tmpl, const tls_params *params, int64_t median_kernel,
                          tls_power_summary *out_summary, double *out_chi2, int64_t *out_row, double *out_depth,
                          double *out_power, double *out_SR, double *out_power_raw,
                          const double *row_duration, double fill_factor, const double *root, const double *root_count,
                          int64_t n_root,
                          tls_transit_stats *out_stats, int64_t max_epochs, double *out_per_transit,
                          int64_t *out_n_epochs,
                          int64_t k, double min_separation, const double *ratios, int64_t n_ratios, double min_power,
                          tls_peak *out_peaks /* [n_curves][k] */, int64_t *out_n_peaks /* [n_curves] */);

/* ---- survey mode: the final T0 fit and the vetting statistics of every peak ------------------------------------------ */
/* What the chain behind the search gives the one pick of a light curve, for one of its peaks: 18 doubles. */
typedef struct tls_peak_fit {
    double T0;       /* tls_first_min over the candidate's trial epochs; NaN when status != 0 */
    double status;   /* 0 fitted; 1 no such peak (rank >= n_peaks); 2 the search fitted nothing at this index (row < 0) */
    tls_transit_stats stats;   /* as the best pick's, from (period, depth, row, index) of the peak; NaN when status != 0 */
} tls_peak_fit;
/* tls_power_batch_peaks plus, for every peak of every light curve, the final T0 fit and the statistics record, computed on
 * the device behind each group's peaks and copied back with them (still one wait per group).  A candidate takes period,
 * depth AND template row from its own index (tls_peak.row); the best pick takes its row from argmin(chi2) and period and
 * depth from argmax(power), so the first peak's fit equals the summary's T0 and out_stats exactly where index_best ==
 * index_power.  The period-uncertainty walk starts at the peak's index.  Summary, statistics and peaks are those of
 * tls_power_batch_peaks, bit for bit.  row_duration, fill_factor, root, root_count, n_root and max_epochs are read even when
 * out_stats is NULL (then out_per_transit and out_n_epochs are not written); the time stamps must ascend; a candidate with more
 * than max_epochs transit epochs, or whose row is not the first row of a template duration, is TLS_E_ARG.  The fits run
 * in slabs of at most 128 (device memory: DESIGN.md "Peak fits").  out_fits [n_curves][k]. */
int tls_power_batch_peak_fits(tls_ctx *ctx, const double *t, const double *y, const double *dy, int64_t n,
                              int64_t n_curves, const double *periods, int64_t n_periods,
                              const tls_template *tmpl, const tls_params *params, int64_t median_kernel,
                              tls_power_summary *out_summary, double *out_chi2, int64_t *out_row, double *out_depth,
                              double *out_power, double *out_SR, double *out_power_raw,
                              const double *row_duration, double fill_factor, const double *root, const double *root_count,
                              int64_t n_root,
                              tls_transit_stats *out_stats, int64_t max_epochs, double *out_per_transit,
                              int64_t *out_n_epochs,
                              int64_t k, double min_separation, const double *ratios, int64_t n_ratios, double min_power,
                              tls_peak *out_peaks /* [n_curves][k] */, int64_t *out_n_peaks /* [n_curves] */,
                              tls_peak_fit *out_fits /* [n_curves][k] */);
/* Developer/test entry: the same stage on the prepared plan (tls_prepare) with injected peak records -- light curves
 * y [n_curves][n], peaks [n_curves][k] of which the first n_peaks[c] count (index in [0, n_periods), row in [-1, n_rows);
 * power is not read from the records), the detrended power [n_curves][n_periods] the period-uncertainty walk reads, and
 * the statistics inputs.  out_fits [n_curves][k]; out_epochs and out_residuals (each NULL or [n_curves][k][n]) and
 * out_n_epochs (NULL or [n_curves][k]) return every fit's trial epochs, as tls_debug_post_search does.  n_curves in
 * [1, 1024]. */
int tls_debug_peak_fits(tls_ctx *ctx, const double *y, int64_t n_curves, const tls_peak *peaks, const int64_t *n_peaks,
                        int64_t k, const double *power, const double *row_duration, int64_t n_rows, double fill_factor,
                        const double *root, const double *root_count,
                        int64_t n_root, int64_t max_epochs, tls_peak_fit *out_fits,
                        double *out_epochs, double *out_residuals, int64_t *out_n_epochs);

/* ---- survey mode: the secondary-eclipse phase scan of a candidate --------------------------------------------------- */
/* The test against an eclipsing binary found at its true period: fold the light curve at (period, T0), measure the depth of
 * a box of about one transit duration at every phase, and report the primary box, the deepest box away from it (the
 * secondary candidate), the most negative one (a brightening) and the scatter of the box depths -- the empirical noise of
 * such a box, red noise included.  Unweighted.  For a candidate (y [n] over t [n], P, T0, d = duration in days):
 *   status 1 and NaN in every other field unless P, T0, d are finite, P > 0, d > 0 and q = 2.0 * P / d >= 16
 *   B = int(min(floor(q), max_bins))                        bins of width 1/B >= d/(2P)
 *   for i ascending:  x = (t[i] - T0) / P;  phi = x - floor(x);  b = min(int(phi * B), B - 1);  S[b] += y[i];  N[b] += 1
 *   window j = bins j and (j+1) % B:  W[j] = S[j] + S[(j+1)%B],  M[j] = N[j] + N[(j+1)%B];  primary window p = B-1
 *   baseline Sb, Nb: bins 2 .. B-3 summed ascending;  inside windows: 2 <= j <= B-4
 *   delta[j] = (Sb - W[j]) / (Nb - M[j]) - W[j] / M[j]      inside j with M[j] >= min_count and Nb - M[j] >= 1
 *   delta[p] = Sb / Nb - W[p] / M[p]                        if M[p] >= min_count and Nb >= 1;  every other delta NaN
 *   js / jb = the first inside j of the largest / smallest delta that is no NaN (none: n_windows = 0, the rest NaN)
 *   rest = those j with |j - js| > 2;  n_windows = len(rest);  where n_windows >= 8:
 *   scan_mean = mu = sum(delta over rest, ascending) / n_windows;  scan_std = sqrt(sum((delta - mu)^2, ascending) / n_windows)
 * Every step is one IEEE double operation and every sum runs in the stated order: the record equals the Python statement
 * in tests/phase_scan_spec.py bit for bit.  The time stamps must be finite.  Counts are doubles.  12 doubles. */
#define TLS_PHASE_SCAN_MIN_BINS 16
#define TLS_PHASE_SCAN_MAX_BINS 4096
typedef struct tls_phase_record {
    double status;                 /* 0 scanned; 1 nothing to scan (no such fit, a bad candidate, or fewer than 16 bins) */
    double n_bins, n_windows;      /* B; windows the scatter was taken over */
    double primary_depth, primary_count;                        /* delta[p], M[p] */
    double secondary_depth, secondary_phase, secondary_count;   /* delta[js], (js + 1) / B, M[js] */
    double bump_depth, bump_phase;                              /* delta[jb], (jb + 1) / B */
    double scan_mean, scan_std;
} tls_phase_record;
/* The scans of n_fits candidates the caller holds: fit f is light curve curve[f] of y [n_curves][n] over t [n] at
 * (period[f], T0[f], duration[f] in days); out [n_fits].  Needs no plan and no search, and leaves a prepared plan as it is.
 * n_fits == 0 is a no-op.  TLS_E_ARG when a curve[f] is outside [0, n_curves), max_bins outside [16, 4096], min_count < 1
 * or a time stamp is not finite.  The device holds the whole batch during the call. */
int tls_phase_scan(tls_ctx *ctx, const double *t, const double *y, int64_t n, int64_t n_curves, const int64_t *curve,
                   const double *period, const double *T0, const double *duration, int64_t n_fits, int64_t max_bins,
                   int64_t min_count, tls_phase_record *out);
/* tls_power_batch_peak_fits plus the phase scan of every peak, on the device behind each slab's fits, from the period, T0
 * and duration_days of the fit records there; the records ride in the group's one copy, 96 bytes a peak.  A fit of
 * status != 0 gives a scan of status 1.  Summary, statistics, peaks and fits are those of tls_power_batch_peak_fits, bit
 * for bit.  out_scans [n_curves][k]. */
int tls_power_batch_phase_scan(tls_ctx *ctx, const double *t, const double *y, const double *dy, int64_t n,
                               int64_t n_curves, const double *periods, int64_t n_periods,
                               const tls_template *tmpl, const tls_params *params, int64_t median_kernel,
                               tls_power_summary *out_summary, double *out_chi2, int64_t *out_row, double *out_depth,
                               double *out_power, double *out_SR, double *out_power_raw,
                               const double *row_duration, double fill_factor, const double *root, const double *root_count,
                               int64_t n_root,
                               tls_transit_stats *out_stats, int64_t max_epochs, double *out_per_transit,
                               int64_t *out_n_epochs,
                               int64_t k, double min_separation, const double *ratios, int64_t n_ratios, double min_power,
                               tls_peak *out_peaks /* [n_curves][k] */, int64_t *out_n_peaks /* [n_curves] */,
                               tls_peak_fit *out_fits /* [n_curves][k] */, int64_t max_bins, int64_t min_count,
                               tls_phase_record *out_scans /* [n_curves][k] */);
/* Developer/test entry: tls_debug_peak_fits (without the fits' epochs) plus the phase scan of every injected peak record,
 * as tls_power_batch_phase_scan runs it behind the fits.  out_scans [n_curves][k]. */
int tls_debug_peak_phase_scans(tls_ctx *ctx, const double *y, int64_t n_curves, const tls_peak *peaks, const int64_t *n_peaks,
                               int64_t k, const double *power, const double *row_duration, int64_t n_rows,
                               double fill_factor, const double *root, const double *root_count,
                               int64_t n_root, int64_t max_epochs,
                               tls_peak_fit *out_fits, int64_t max_bins, int64_t min_count, tls_phase_record *out_scans);

/* ---- survey mode: single-transit events ------------------------------------------------------------------------------ */
/* The unfolded search: a planet that transits once in the window has no periodogram peak.  A template of every trial width
 * slides along the time series itself.  For a curve (y [n], dy [n] over the ascending, finite t [n]), n_rows rows of strictly
 * ascending widths L_r in [3, TLS_SINGLE_MAX_WIDTH] samples with shapes b_r[j] (0 out of transit, 1 at the bottom; row r is
 * shape_values[shape_offset[r] .. + L_r)), span_max[r] in days and depth_min >= 0:
 *   w = 1.0 / (dy * dy);  xw = (1.0 - y) * w;  bb_r[j] = b_r[j] * b_r[j]
 *   for every centre c in 0..n-1, rows r ascending (nothing held at first):
 *       h = (L_r - 1) / 2;  lo = c - h;  hi = lo + L_r - 1
 *       skip if lo < 0 or hi > n - 1 or not (t[hi] - t[lo] <= span_max[r])           the window runs over a gap
 *       N = 0; D = 0; for j = 0..L_r-1 ascending: N = N + xw[lo+j] * b_r[j];  D = D + w[lo+j] * bb_r[j]
 *       d = N / D;  skip if not (d > depth_min)                                      least-squares depth; dips only
 *       s = N / sqrt(D);  take (s, r, d) if nothing is held or s > held s            the first row wins ties
 *   ses[c], row[c], depth[c] = held, or NaN, -1, NaN
 * Events, at most k: a centre is alive where ses[c] is no NaN and ses[c] >= min_ses; its window is [lo, hi] of its own best
 * row.  Repeat: the alive centre of the largest ses (the lowest index on ties) is taken; with g = int(separation * L) of its
 * row, every alive centre whose window meets [lo - g, hi + g] leaves (integers only).  Stop at k events or when nothing is
 * alive.  Every step is one IEEE double operation and every sum runs in the stated order: planes and records equal the Python
 * statement in tests/single_transit_spec.py bit for bit.  8 doubles; ranks past a curve's n_events hold index -1 and NaN. */
#define TLS_SINGLE_MAX_WIDTH 4096
#define TLS_SINGLE_MAX_K 32
typedef struct tls_single_event {
    double index, time;            /* c, t[c] */
    double ses, depth;             /* s and d of the centre's best row */
    double row, width;             /* r, L_r */
    double t_first, t_last;        /* t[lo], t[hi] */
} tls_single_event;
/* The events of n_curves curves y, dy [n_curves][n] on the shared time stamps t [n]: out_events [n_curves][k], out_n_events
 * [n_curves]; out_ses, out_depth (double) and out_row (int64) [n_curves][n] are the planes, each NULL (not returned: they stay
 * in the context's device scratch) or given.  Needs no plan and no search, and leaves a prepared plan as it is.  n_curves == 0
 * is a no-op.  TLS_E_ARG, before any device work and with the outputs untouched, for n outside [1, 2^20], negative counts,
 * n_rows < 1, widths not strictly ascending or outside [3, TLS_SINGLE_MAX_WIDTH], a negative shape_offset, k outside
 * [1, TLS_SINGLE_MAX_K], a non-finite or negative depth_min, separation or span_max, a NaN min_ses, and a t that is not
 * finite and non-decreasing.  y and dy are taken as they are (dy > 0). */
int tls_single_transits(tls_ctx *ctx, const double *t, const double *y, const double *dy, int64_t n, int64_t n_curves,
                        const double *shape_values, const int64_t *shape_offset, const int64_t *width, const double *span_max,
                        int64_t n_rows, double depth_min, int64_t k, double min_ses, double separation,
                        tls_single_event *out_events, int64_t *out_n_events, double *out_ses, int64_t *out_row,
                        double *out_depth);

/* ---- survey mode: individual transit times and a refitted ephemeris ---------------------------------------------------- */
/* The transit-by-transit view of a candidate: every transit of a linear ephemeris (P, T0) is timed on its own with the
 * template of the candidate's duration, and the straight line through the times gives a refined (period, T0) with errors that
 * come from the transits themselves, the observed-minus-computed times and their chi^2.  For a curve (y [n], dy [n] over the
 * ascending, finite t [n]), a candidate (P, T0, row r, reach S >= 1), row r of L in [3, TLS_SINGLE_MAX_WIDTH] samples with the
 * shape b[j] (0 out of transit, 1 at the bottom; shape_values[shape_offset[r] .. + L)) and span_max in days, depth_min >= 0:
 *   w = 1.0 / (dy * dy);  xw = (1.0 - y) * w
 *   bb[j] = b[j]*b[j];  g[j] = 0.5 * (b[j+1] - b[j-1]) with b[-1] = b[L] = 0.0;  gg[j] = g[j]*g[j];  bg[j] = b[j]*g[j];  h = (L-1)/2
 *   status 1 and NaN in every other field unless P and T0 are finite and P > 0
 *   e_first = ceil((t[0] - T0) / P);  e_last = floor((t[n-1] - T0) / P);  n_epochs = (e_last - e_first) + 1.0       (doubles)
 *   status 2 unless 1 <= n_epochs <= max_epochs: n_epochs is reported, the rest is NaN
 *   every epoch e = e_first + i, i = 0 .. n_epochs-1:
 *       tc = T0 + e * P;  j = first index with t[j] >= tc (n-1 if there is none)
 *       if j > 0 and tc - t[j-1] <= t[j] - tc:  j = j - 1                             the nearer sample; the lower one on a tie
 *       for s = -S .. S ascending:  c = j + s;  lo = c - h;  hi = lo + L - 1
 *           skip if lo < 0 or hi > n-1 or not (t[hi] - t[lo] <= span_max)              the window runs over a gap
 *           N = 0; D = 0; for k ascending:  N = N + xw[lo+k]*b[k];  D = D + w[lo+k]*bb[k]
 *           d = N / D;  skip if not (d > depth_min);  q = N / sqrt(D)
 *           hold (q, d, c, lo) if nothing is held or q > held q                        the first shift wins ties
 *       nothing held: epoch status 1, time_linear = tc, the rest NaN
 *       ses = q, depth = d, index = c;  tm = 0.5 * (t[lo+h] + t[lo+L-1-h])             the window's centre; t[c] for odd L
 *       epoch status 3 if not (q >= min_ses)                                           too weak to time
 *       epoch status 2 if c-1 < 0 or c+1 > n-1
 *       H = 0; Bg = 0; G = 0; for k ascending:  H = H + xw[lo+k]*g[k];  Bg = Bg + w[lo+k]*bg[k];  G = G + w[lo+k]*gg[k]
 *       delta = (d*Bg - H) / (d*G);  step = 0.5 * (t[c+1] - t[c-1])                    one Gauss-Newton step of the shift
 *       epoch status 2 if not (fabs(delta) <= 1.0)                                     the step leaves the sample (NaN, G == 0)
 *       epoch status 0:  time = tm + delta*step;  time_err = step / (d * sqrt(G))
 *   over the epochs of status 0, ascending:  wgt = 1.0/(time_err*time_err);  x = e;  tau = time - T0
 *       Sw += wgt;  Se += wgt*x;  See += (wgt*x)*x;  St += wgt*tau;  Set += (wgt*x)*tau;  Dl = Sw*See - Se*Se
 *   where n_timed >= 2 and Dl > 0:  slope = (Sw*Set - Se*St)/Dl;  icpt = (See*St - Se*Set)/Dl
 *       period = slope;  T0 = T0 + icpt;  period_err = sqrt(Sw/Dl);  T0_err = sqrt(See/Dl)
 *   where also n_timed >= 3:  oc = tau - (icpt + slope*x);  rr = oc/time_err;  chi2 += rr*rr;  ss += oc*oc
 *       ttv_chi2 = chi2;  ttv_rms = sqrt(ss / n_timed);  ttv_max_sigma, ttv_max_epoch = the largest fabs(rr), its epoch (the first)
 * Everything that cannot be formed is NaN.  time_err is the Fisher bound of the shape at the fitted depth on white noise of
 * the given dy: red noise and a wrong shape make the true scatter larger, which ttv_chi2 of a quiet star shows.  Every step is
 * one IEEE double operation and every sum runs in the stated order: both records equal the Python statement in
 * tests/transit_times_spec.py bit for bit.  All fields are doubles. */
#define TLS_TIMES_MAX_REACH 4096
#define TLS_TIMES_MAX_EPOCHS 65536
typedef struct tls_ephemeris {
    double status;                 /* 0 epochs were looked at; 1 no such ephemeris (P, T0); 2 n_epochs outside [1, max_epochs] */
    double n_epochs, n_timed;      /* epochs inside the series; those of epoch status 0 */
    double epoch_first;            /* e_first */
    double period, period_err;     /* slope and its error (n_timed >= 2) */
    double T0, T0_err;             /* T0 + intercept and its error */
    double ttv_chi2, ttv_rms;      /* chi^2 and root mean square of the observed-minus-computed times (n_timed >= 3) */
    double ttv_max_sigma, ttv_max_epoch;   /* the largest |o - c| / time_err and its epoch */
} tls_ephemeris;
typedef struct tls_transit_time {
    double epoch;                  /* e; NaN at ranks past n_epochs */
    double status;                 /* 0 timed; 1 no window with a dip (a gap, an end of the series); 2 found but not timed: the
                                      step leaves the sample or the series; 3 found but weaker than min_ses */
    double time_linear;            /* tc */
    double time, time_err;         /* status 0 */
    double ses, depth, index;      /* q, d, c of the held window (status 0, 2, 3) */
} tls_transit_time;
/* n_fits candidates (period[f], T0[f], row[f], reach[f]) on the curves curve[f] of y, dy [n_curves][n] over the shared time
 * stamps t [n]; the rows as tls_single_transits takes them.  out [n_fits], out_times [n_fits][max_epochs].  Needs no plan and no
 * search, and leaves a prepared plan as it is.  n_fits == 0 is a no-op.  Candidates are processed in slabs, so device memory
 * stays bounded for any n_fits.  TLS_E_ARG, before any device work and with the outputs untouched, for a curve[f] outside
 * [0, n_curves), a row[f] outside [0, n_rows), a reach[f] outside [1, TLS_TIMES_MAX_REACH], max_epochs outside
 * [1, TLS_TIMES_MAX_EPOCHS], n outside [1, 2^30], negative counts, n_rows < 1, widths not strictly ascending or outside
 * [3, TLS_SINGLE_MAX_WIDTH], a negative shape_offset, a non-finite or negative span_max or depth_min, a NaN min_ses, and a t
 * that is not finite and non-decreasing.  y and dy are taken as they are (dy > 0). */
int tls_transit_times(tls_ctx *ctx, const double *t, const double *y, const double *dy, int64_t n, int64_t n_curves,
                      const int64_t *curve, const double *period, const double *T0, const int64_t *row, const int64_t *reach,
                      int64_t n_fits, const double *shape_values, const int64_t *shape_offset, const int64_t *width,
                      const double *span_max, int64_t n_rows, double depth_min, double min_ses, int64_t max_epochs,
                      tls_ephemeris *out /* [n_fits] */, tls_transit_time *out_times /* [n_fits][max_epochs] */);

/* ---- survey mode: the period aliases of two- and few-transit events ---------------------------------------------------- */
/* Two single-transit events of a star (two sectors a year apart, a campaign with a gap) have no periodogram peak, but they fix
 * the period up to the aliases P_k = (t_b - t_a) / k, and the data decide among them: an alias is ruled out when one of its
 * other epochs falls on good data that show no dip, allowed when they all fall in gaps, confirmed when another one shows a dip.
 * For a curve (y [n], dy [n] over the ascending, finite t [n]) and the rows of tls_transit_times (L, b, span_max), a pair is
 * (ca < cb sample indices, row r, reach S >= 1, offset >= 0 days):
 *   w = 1.0 / (dy * dy);  xw = (1.0 - y) * w;  bb[j] = b[j]*b[j];  h = (L-1)/2
 *   window(c):  lo = c - h;  hi = lo + L - 1;  invalid if lo < 0 or hi > n-1 or not (t[hi] - t[lo] <= span_max)
 *               N = 0; D = 0; for j ascending:  N = N + xw[lo+j]*b[j];  D = D + w[lo+j]*bb[j]
 *   look(tc):   j = first index with t[j] >= tc (n-1 if there is none)
 *               if j > 0 and tc - t[j-1] <= t[j] - tc:  j = j - 1                      tls_transit_times' nearest sample
 *               for s = -S .. S ascending:  c = j + s
 *                   skip if c < 0 or c > n-1, or window(c) is invalid
 *                   skip if not (fabs(t[c] - tc) <= offset)                             a centre at the edge of a gap covers no epoch inside it
 *                   skip if not (D > 0);  q = N / sqrt(D)                               signed, NO depth_min test: a missing dip must count
 *                   hold (q, N, D) if nothing is held or q > held q                     the first shift wins ties
 *               nothing held: the epoch is uncovered
 *   ta = t[ca];  tb = t[cb];  dT = tb - ta;  status 1 unless dT > 0                     dT is reported, the rest is NaN
 *   A = look(ta);  B = look(tb);  status 2 unless both are covered and N_A + N_B > 0    dT; pair_mes, pair_depth where both are covered
 *   pN = N_A + N_B;  pD = D_A + D_B;  pair_depth = pN / pD;  pair_mes = pN / sqrt(pD)
 *   k_hi = floor(dT / period_min);  n_aliases = k_hi;  status 3 if k_hi < 1             n_evaluated = n_allowed = 0, no alias
 *   n_evaluated = min(k_hi, max_aliases)
 *   alias k = 1 .. n_evaluated:
 *       P = dT / k;  e_first = ceil((t[0] - ta) / P);  e_last = floor((t[n-1] - ta) / P);  n_epochs = (e_last - e_first) + 1.0
 *       SN = 0; SD = 0; n_covered = 0; n_seen = 0; worst_sigma = NaN; worst_epoch = NaN
 *       for e = e_first + i, i = 0 .. n_epochs-1:
 *           tc = ta + e * P;  look(tc);  uncovered: next epoch
 *           n_covered += 1;  SN = SN + N;  SD = SD + D;  if q >= min_ses:  n_seen += 1
 *           if e != 0 and e != k:  z = (pair_depth - N / D) * sqrt(D)                   how far the epoch falls short of the pair's depth
 *               if worst_sigma is NaN or z > worst_sigma:  worst_sigma = z;  worst_epoch = e
 *       mes = SN / sqrt(SD);  depth = SN / SD
 *   allowed(k) = not (worst_sigma > veto_sigma)                                         NaN: no other covered epoch, allowed
 *   best = the allowed alias with the largest non-NaN mes (the smallest k on ties, i.e. the longest period)
 *   longest / shortest = the smallest / largest allowed k;  n_allowed = their count
 * Everything that cannot be formed is NaN.  Every step is one IEEE double operation and every sum runs in the stated order:
 * both records equal the Python statement in tests/event_periods_spec.py bit for bit.  All fields are doubles. */
#define TLS_ALIAS_MAX 4096
typedef struct tls_event_pair {
    double status;                 /* 0 aliases were looked at; 1 dT <= 0; 2 an event is uncovered or the pair shows no dip; 3 no alias >= period_min */
    double dT;                     /* t[cb] - t[ca] */
    double n_aliases, n_evaluated; /* k_hi; min(k_hi, max_aliases) */
    double n_allowed;
    double pair_mes, pair_depth;   /* of the two events together */
    double best_k, best_period, best_mes, best_n_covered, best_n_seen;
    double longest_k, longest_period;
    double shortest_k, shortest_period;
} tls_event_pair;
typedef struct tls_event_alias {
    double period;                 /* dT / k at rank k - 1; NaN in every field at ranks past n_evaluated */
    double n_epochs, n_covered;    /* epochs inside the series; those a window covers */
    double n_seen;                 /* covered epochs with q >= min_ses */
    double mes, depth;             /* over the covered epochs */
    double worst_sigma, worst_epoch;   /* the largest shortfall of a covered epoch other than the pair's own, and its epoch */
} tls_event_alias;
/* n_pairs pairs (curve[f], index_a[f], index_b[f], row[f], reach[f], offset[f]) on the curves of y, dy [n_curves][n] over the
 * shared time stamps t [n]; the rows as tls_single_transits takes them.  out [n_pairs], out_aliases [n_pairs][max_aliases] (may
 * be NULL).  Needs no plan and no search, and leaves a prepared plan as it is.  n_pairs == 0 is a no-op.  Pairs are processed in
 * slabs, so device memory stays bounded for any n_pairs.  TLS_E_ARG, before any device work and with the outputs untouched, for
 * what tls_transit_times refuses for t, the rows, curve, row and reach, n outside [1, 2^20], an index outside [0, n) or
 * index_a >= index_b, a non-finite or negative offset, a period_min that is not finite and > 0 or has
 * (t[n-1] - t[0]) / period_min + 2 > TLS_TIMES_MAX_EPOCHS, max_aliases outside [1, TLS_ALIAS_MAX], and a NaN min_ses or
 * veto_sigma (+inf is legal: no veto).  y and dy are taken as they are (dy > 0). */
int tls_event_periods(tls_ctx *ctx, const double *t, const double *y, const double *dy, int64_t n, int64_t n_curves,
                      const int64_t *curve, const int64_t *index_a, const int64_t *index_b, const int64_t *row,
                      const int64_t *reach, const double *offset, int64_t n_pairs, const double *shape_values,
                      const int64_t *shape_offset, const int64_t *width, const double *span_max, int64_t n_rows,
                      double period_min, int64_t max_aliases, double min_ses, double veto_sigma,
                      tls_event_pair *out /* [n_pairs] */, tls_event_alias *out_aliases /* [n_pairs][max_aliases], or NULL */);

/* Per-transit event vetting: the tests of a candidate's INDIVIDUAL events (after the Kepler Robovetter's individual transit
 * metrics, Thompson et al. 2018, A.3.7) -- is an event unique in its neighbourhood, does it rest on one sample, does the flux
 * come back to the baseline, does the candidate survive without its bad events or without its strongest one.  The inputs are
 * those of tls_transit_times; a candidate also has a chase reach R >= 0 and a guard Gd >= 0 in samples and a chase_span > 0 in
 * days, the call chase_fraction in (0, 1], chase_min in [0, 1], point_fraction > 0 and step_fraction > 0.
 *   w = 1.0 / (dy * dy);  xw = (1.0 - y) * w;  bb[k] = b[k]*b[k];  h = (L - 1) / 2
 *   candidate status 1 / 2 and n_epochs as tls_transit_times has them
 *   every epoch e = e_first + i:
 *       tc, the nearest sample j and the held window (q, d, c, lo) over the shifts -S .. S as tls_transit_times finds them (the
 *       same skips, the same chains, the first shift wins ties); N, D of the held window are kept
 *       nothing held: event status 1, epoch and time_linear = tc reported, every other field NaN
 *       event status 0:  ses = q;  depth = d;  index = c;  depth_err = 1.0 / sqrt(D)
 *       point:   pm = xw[lo]*b[0];  k = 1 .. L-1 ascending:  v = xw[lo+k]*b[k];  pm = v if v > pm
 *                point_share = pm / N                                  the numerator's share resting on one sample
 *       sides:   before over [lo-L, lo-1], after over [lo+L, lo+2L-1]; for a side [a, z]:
 *                NaN if a < 0 or z > n-1 or not (t[z] - t[a] <= span_max)
 *                Ns = 0; Ws = 0; k ascending:  Ns = Ns + xw[a+k];  Ws = Ws + w[a+k];   side = (Ns / Ws) / d
 *       chase:   n_chased = 0;  found = false
 *                for m = Gd+1 .. R, for c' in (c - m, c + m):  lo' = c' - h;  hi' = lo' + L - 1
 *                    skip if lo' < 0 or hi' > n-1 or not (t[hi'] - t[lo'] <= span_max)
 *                    n_chased += 1;  N', D' as N, D (k ascending);  q' = N' / sqrt(D')
 *                    if fabs(q') >= chase_fraction * q:  dtc = fabs(t[c'] - t[c]);  chase_dt = dtc if not found or dtc < chase_dt
 *                                                        found = true
 *                chases = NaN if n_chased == 0;  1.0 if not found;  else x = chase_dt / chase_span, 1.0 if not (x < 1.0)
 *                chase_dt is NaN unless found
 *       flags = 1 * (not q >= min_ses) + 2 * (point_share > point_fraction)
 *             + 4 * (before > step_fraction or after > step_fraction) + 8 * (chases < chase_min)      NaN compares false
 *       good iff flags == 0
 *   candidate, over the events of status 0 ascending (n_held of them):
 *       SN = SN + N;  SD = SD + D;  mes = SN / sqrt(SD);  depth_mean = SN / SD
 *       ses_max, ses_max_epoch: the largest q and its epoch, the first on ties;  dominance = ses_max / mes
 *       n_good, mes_good: the same two sums over the good events only (NaN where n_good == 0)
 *       mes_rest: the same over the held events except the ses_max epoch (NaN where n_held < 2)
 *       depth_chi2:  r = d_e - depth_mean;  chi2 = chi2 + (r*r)*D_e
 *       chases_min, chases_mean (sum / count, ascending) over the events whose chases is not NaN; NaN if none
 *       n_held == 0: n_held = 0, n_good = 0, the rest NaN (status, n_epochs and epoch_first stay)
 * chase_dt is a minimum of non-negative doubles and n_chased a count, so neither depends on the order the chase windows are
 * visited in; every other sum runs in the stated order and every step is one IEEE double operation: both records equal the
 * Python statement in tests/event_vetting_spec.py bit for bit.  mes is formed from each event's BEST shift, so it is biased
 * upward against a strictly linear ephemeris: compare it with mes_good and mes_rest, not with the search's SNR.  All fields
 * are doubles. */
#define TLS_EVENTS_MAX_CHASE 8192
typedef struct tls_event_summary {
    double status;                 /* 0 epochs were looked at; 1 no such ephemeris (P, T0); 2 n_epochs outside [1, max_epochs] */
    double n_epochs, epoch_first;  /* epochs inside the series; e_first */
    double n_held, n_good;         /* events of status 0; those without a flag */
    double mes, mes_good, mes_rest;    /* SN / sqrt(SD) over the held events, over the good ones, over all but the strongest */
    double ses_max, ses_max_epoch, dominance;   /* the strongest event, its epoch, ses_max / mes */
    double depth_mean, depth_chi2; /* SN / SD, and the chi^2 of the events' depths about it */
    double chases_min, chases_mean;    /* over the events that had a chase window */
} tls_event_summary;
typedef struct tls_event_record {
    double epoch;                  /* e; NaN at ranks past n_epochs */
    double status;                 /* 0 an event is held; 1 no window with a dip (a gap, an end of the series) */
    double time_linear;            /* tc */
    double ses, depth, depth_err, index;   /* q, d, 1 / sqrt(D), c of the held window */
    double point_share;            /* the largest term of N over N: > point_fraction, the event rests on one sample */
    double before, after;          /* the mean dip of the L samples on either side over d: > step_fraction, the flux is not at
                                      the baseline there (a step, a ramp); NaN where the side leaves the series or runs over a gap */
    double chases;                 /* min(chase_dt / chase_span, 1): how far away the nearest comparable event is; 1 none */
    double chase_dt, n_chased;     /* days to the nearest comparable window (NaN: none); windows looked at */
    double flags;                  /* 1 weaker than min_ses | 2 point | 4 step | 8 chased */
} tls_event_record;
/* n_fits candidates (period[f], T0[f], row[f], reach[f], chase_reach[f], guard[f], chase_span[f]) on the curves curve[f]; the
 * other arguments as tls_transit_times takes them.  out [n_fits], out_events [n_fits][max_epochs].  Needs no plan and no
 * search, and leaves a prepared plan as it is.  n_fits == 0 is a no-op.  Candidates are processed in slabs, so device memory
 * stays bounded for any n_fits.  TLS_E_ARG, before any device work and with the outputs untouched, for everything
 * tls_transit_times rejects, and for a chase_reach[f] outside [0, TLS_EVENTS_MAX_CHASE], a negative guard[f], a chase_span[f]
 * that is not finite and > 0, chase_fraction outside (0, 1], chase_min outside [0, 1], and a point_fraction or step_fraction
 * that is not > 0 (NaN included). */
int tls_event_vetting(tls_ctx *ctx, const double *t, const double *y, const double *dy, int64_t n, int64_t n_curves,
                      const int64_t *curve, const double *period, const double *T0, const int64_t *row, const int64_t *reach,
                      const int64_t *chase_reach, const int64_t *guard, const double *chase_span, int64_t n_fits,
                      const double *shape_values, const int64_t *shape_offset, const int64_t *width, const double *span_max,
                      int64_t n_rows, double depth_min, double min_ses, double chase_fraction, double chase_min,
                      double point_fraction, double step_fraction, int64_t max_epochs,
                      tls_event_summary *out /* [n_fits] */, tls_event_record *out_events /* [n_fits][max_epochs] */);

/* The shape of a candidate's dip: a trapezoid of unit depth -- total duration T (T14), flat bottom T (1 - 2 g), g = T12/T14,
 * centre shifted by c0 -- is fitted to the points around every transit of a linear ephemeris, over a grid of durations,
 * ingress fractions and shifts, with the baseline fixed at 1.  A box is g = 0, a V is g = 0.5.  For a curve (y [n], dy [n]
 * over the ascending, finite t [n]), a candidate (P, T0, d in days) and the ascending tables ratio[nT] > 0, ingress[nQ] with
 * ingress[0] == 0.0 and ingress[nQ-1] == 0.5, shift[nS]:
 *   w = 1.0 / (dy * dy);  xw = (1.0 - y) * w
 *   status 1 and NaN in every other field unless P, T0, d are finite, P > 0, d > 0 and wd = window * d < 0.5 * P
 *   members, i ascending:  x = (t[i] - T0) / P;  k = floor(x + 0.5);  tau = (x - k) * P;  member iff fabs(tau) <= wd
 *   unit (a, b, c), a outermost, c innermost (unit index (a * nQ + b) * nS + c):
 *       T = d * ratio[a];  ho = 0.5 * T;  hb = ho * (1.0 - 2.0 * ingress[b]);  r = 1.0 / (ho - hb) where hb < ho;  c0 = d * shift[c]
 *       cnt = 0; N = 0; D = 0; over the members in index order:  u = fabs(tau - c0)
 *           s = 1.0 if u <= hb, else (ho - u) * r if u < ho, else the member does not count
 *           cnt += 1;  N = N + xw * s;  s2 = s * s;  D = D + w * s2
 *       valid iff cnt >= min_count and D > 0 and dep = N / D > depth_min;  q = N / sqrt(D)
 *   best = the valid unit of the largest q, the first in unit order among equals; box and vee = the same pick among the units
 *   with b == 0 and with b == nQ - 1;  status 2 (n_points reported, the rest NaN) if no unit is valid.
 * ses^2 - ses_vee^2 is the chi^2 by which the best trapezoid beats the best V; ses_box^2 - ses_vee^2 has the sign of the shape.
 * The trapezoid knows nothing of limb darkening or exposure time: `ingress` of a planet is larger than its geometric T12/T14.
 * Every step is one IEEE double operation and every sum runs in index order: the record equals the Python statement in
 * tests/shape_fit_spec.py bit for bit.  All fields are doubles. */
#define TLS_SHAPE_MAX_UNITS 65536
typedef struct tls_shape_record {
    double status;                 /* 0 fitted; 1 no such candidate (P, T0, d, or a window of half a period or more); 2 no valid unit */
    double n_points;               /* the members */
    double n_in;                   /* cnt of the best unit */
    double ses, depth, depth_err;  /* q, N / D and 1 / sqrt(D) of the best unit */
    double duration, ingress, shift;           /* T (days), ingress[b] (T12/T14), c0 (days) of the best unit */
    double i_duration, i_ingress, i_shift;     /* a, b, c */
    double ses_box, duration_box;  /* q and T of the best unit with b == 0 */
    double ses_vee, duration_vee;  /* q and T of the best unit with b == nQ - 1 */
} tls_shape_record;
/* n_fits candidates (period[f], T0[f], duration[f]) on the curves curve[f] of y, dy [n_curves][n] over the shared time stamps
 * t [n].  out [n_fits].  Needs no plan and no search, and leaves a prepared plan as it is.  n_fits == 0 is a no-op.
 * Candidates are processed in slabs, so device memory stays bounded for any n_fits.  TLS_E_ARG, before any device work and
 * with the output untouched, for a curve[f] outside [0, n_curves), n outside [1, 2^22], negative counts, an empty table,
 * nT * nQ * nS above TLS_SHAPE_MAX_UNITS, a table that is not finite and non-decreasing, a ratio <= 0, ingress[0] != 0.0 or
 * ingress[nQ-1] != 0.5, a window that is not finite or below 0.5 * ratio[nT-1] + max(fabs(shift[0]), fabs(shift[nS-1])) (the
 * model must lie inside the window), min_count < 1, a non-finite or negative depth_min, and a t that is not finite and
 * non-decreasing.  y and dy are taken as they are (dy > 0); period, T0 and duration may hold any value (status 1). */
int tls_shape_fit(tls_ctx *ctx, const double *t, const double *y, const double *dy, int64_t n, int64_t n_curves,
                  const double *period, const double *T0, const double *duration, const int64_t *curve, int64_t n_fits,
                  const double *ratio, int64_t nT, const double *ingress, int64_t nQ, const double *shift, int64_t nS,
                  double window, int64_t min_count, double depth_min, tls_shape_record *out /* [n_fits] */);

/* The centroid-shift test: WHICH star dims.  A background eclipsing binary a few pixels from the target, diluted to a
 * planet-like depth, passes every test of the flux alone; the flux-weighted photocentre of the aperture (MOM_CENTR1/2 of a
 * Kepler, K2 or TESS light-curve file, on the flux's own time stamps) moves in transit when the dimming source is not at the
 * photocentre (Bryson et al. 2013, PASP 125, 889; Twicken et al. 2018, PASP 130, 064502).  The transit template at the
 * candidate's ephemeris is regressed on three series -- the flux deficit 1 - y, the column centroid cx and the row centroid
 * cy -- over the points within `window` durations of every transit, with a free baseline in every epoch (centroids drift
 * with the pointing).  For a curve (y, cx, cy [n]) over the ascending, finite t [n], a candidate (P, T0, d in days) and the
 * shape b [L] (1 - the limb-darkened reference transit: 0 out of transit, 1 at the bottom):
 *   status 1 and NaN in every other field unless P, T0, d finite, P > 0, d > 0 and wd = window * d < 0.5 * P
 *   points, i ascending:  x = (t[i] - T0) / P;  k = floor(x + 0.5);  tau = (x - k) * P
 *       member iff fabs(tau) <= wd and cx[i], cy[i] both finite;  its epoch is k
 *       v = tau / d + 0.5;  inside iff 0 <= v <= 1
 *       s = 0.0 if not inside, else  u = v * (L - 1);  j = min(floor(u), L - 2);  fr = u - j;  s = b[j] + (b[j+1] - b[j]) * fr
 *   status 2 (n_points = the members, the rest NaN) if the epochs holding a member are more than max_epochs
 *   epoch k, its members in index order:  m = count;  m_in = count(inside);  used iff m_in >= min_in and m - m_in >= min_out
 *       Ss = Ss + s;  sbar = Ss / m;  for each channel c in (1 - y, cx, cy):  Sc = Sc + c;  cbar = Sc / m          (pass 1)
 *       ds = s - sbar;  De = De + ds * ds;  dc = c - cbar;  Ne[c] = Ne[c] + ds * dc;  Qe[c] = Qe[c] + dc * dc      (pass 2)
 *   used epochs ascending:  D = D + De;  N[c] = N[c] + Ne[c];  Q[c] = Q[c] + Qe[c];  n_points += m;  n_in += m_in
 *   status 2 (n_epochs, n_skipped, n_points, n_in reported, the rest NaN) unless n_used >= 1 and D > 0
 *   A[c] = N[c] / D;  dof = n_points - n_used - 1
 *   var[c] = (Q[c] - A[c] * N[c]) / dof where dof >= 1 and that is > 0, else NaN
 *   err[c] = sqrt(var[c] / D);  rms[c] = sqrt(var[c])
 *   chi2[c] = sum over the used epochs with De > 0, ascending, of  r = Ne[c] / De - A[c];  (r * r) * De,  then / var[c]
 * A linear drift across a window is orthogonal to the symmetric template, so the constant of an epoch is enough for a slow
 * pointing drift, and what it leaves inflates rms, not the shift.  chi2 has n_epochs - 1 degrees of freedom: a shift that
 * one event carries is a systematic, not a source.  Every step is one IEEE double operation in the stated order: the record
 * equals the Python statement in tests/centroid_spec.py bit for bit.  All fields are doubles. */
#define TLS_CENTROID_MAX_EPOCHS 65536
#define TLS_CENTROID_MAX_SHAPE 1048576
typedef struct tls_centroid_record {
    double status;                 /* 0 measured; 1 no such candidate (P, T0, d, or a window of half a period or more); 2 too
                                      many epochs, no usable epoch, or no point on the template's slope */
    double n_epochs, n_skipped;    /* the used epochs; epochs with members that are not used */
    double n_points, n_in;         /* members of the used epochs; those inside the transit */
    double depth, depth_err;       /* A, err of 1 - y: the depth measured on the same points in the same way */
    double shift_x, shift_x_err;   /* A, err of cx: the in-transit shift of the photocentre, in the unit of cx */
    double shift_y, shift_y_err;   /* of cy */
    double rms_x, rms_y;           /* the scatter of the centroid residuals */
    double chi2_depth, chi2_x, chi2_y;     /* the epochs' own amplitudes about the common one */
} tls_centroid_record;
/* n_fits candidates (period[f], T0[f], duration[f]) on the curves curve[f] of y, cx, cy [n_curves][n] over the shared time
 * stamps t [n]; shape [L].  out [n_fits].  Needs no plan and no search, and leaves a prepared plan as it is.  n_fits == 0 is
 * a no-op.  Candidates are processed in slabs, so device memory stays bounded for any n_fits.  TLS_E_ARG, before any device
 * work and with the output untouched, for a curve[f] outside [0, n_curves), n outside [1, 2^22], negative counts, L outside
 * [2, TLS_CENTROID_MAX_SHAPE], a shape value that is not finite, a window that is not finite and >= 1, min_in < 1,
 * min_out < 1, max_epochs outside [1, TLS_CENTROID_MAX_EPOCHS], and a t that is not finite and non-decreasing.  y is taken
 * as it is (finite); cx and cy may hold NaN and infinities (the point is skipped); period, T0 and duration may hold any
 * value (status 1). */
int tls_centroid_test(tls_ctx *ctx, const double *t, const double *y, const double *cx, const double *cy, int64_t n,
                      int64_t n_curves, const double *period, const double *T0, const double *duration, const int64_t *curve,
                      int64_t n_fits, const double *shape, int64_t L, double window, int64_t min_in, int64_t min_out,
                      int64_t max_epochs, tls_centroid_record *out /* [n_fits] */);

/* The folded views of a candidate: its light curve folded at the ephemeris and binned by the MEDIAN on a fixed number of
 * bins -- the "global view" and "local view" of Shallue & Vanderburg (2018, AJ 155, 94), and the even, odd and
 * secondary-eclipse local views Valizadegan et al. (2022, ApJ 926, 120) add to them: what a data-validation report plots and
 * a neural-net vetter reads.  For a row y [n] over the ascending, finite t [n], a candidate (P, T0, d in days, phi_s) and a
 * view (phi_c, x_min, x_max, w, B, parity):
 *   points, i ascending:  x = (t[i] - T0) / P;  u = x - phi_c;  e = floor(u + 0.5);  tau = (u - e) * P
 *   bin b, 0 <= b < B:    s = ((x_max - x_min) - w) / (B - 1);  lo = b * s + x_min;  hi = lo + w
 *                         member iff lo <= tau and tau < hi (and, with a parity, e - 2.0 * floor(e / 2.0) == parity)
 *   count[b] = the members;  median[b] = the middle member by value (count odd), (a + b) / 2.0 of the two middle ones (even),
 *   NaN (none);  n_members = the points that are a member of at least one bin
 * Nothing but those two comparisons decides membership: with w > s a point is in several bins, with w < s maybe in none.
 * The five views, with k = local_durations and width = local_width:
 *   global      (0.0,   -0.5 * P, 0.5 * P, P / n_global, n_global, none)
 *   local       (0.0,   -(k * d), k * d,   width * d,    n_local,  none)
 *   local_even  the same with parity 0.0: the transits of even e -- T0 the fit's own: the first, third, ... transit of the
 *               series, power()'s transit_depths[::2] and depth_mean_even;  local_odd with parity 1.0
 *   secondary   the local view about phi_c = phi_s
 * status 1 (every median NaN, every count 0, every n_* 0) unless P, T0, d are finite, P > 0 and d > 0; secondary_status 1 and
 * the secondary view alone NaN / 0 where phi_s is not finite or secondary_phase is NULL.  Every step is one IEEE double
 * operation and a median is a selection: records and arrays equal the Python statement in tests/folded_views_spec.py bit for
 * bit.  All fields are doubles. */
#define TLS_VIEWS_MAX_BINS 65536
typedef struct tls_views_record {
    double status;                 /* 0 binned; 1 no such candidate */
    double secondary_status;       /* 0 binned; 1 no secondary view (no candidate, or no finite phi_s) */
    double n_global, n_local, n_local_even, n_local_odd, n_secondary;   /* n_members of the five views */
} tls_views_record;
/* n_fits candidates (period[f], T0[f], duration[f], secondary_phase[f]; secondary_phase NULL: no secondary view) on the rows
 * curve[f] (NULL: candidate f is curve f) of y [n_curves][n] over the shared time stamps t [n].  out [n_fits];
 * global_median, global_count [n_fits][n_global]; local_median, local_count [n_fits][4][n_local] in the order local,
 * local_even, local_odd, secondary.  The device writes every entry.  Needs no plan and no search, and leaves a prepared plan
 * as it is.  n_fits == 0 is a no-op.  Candidates are processed in slabs, so device memory stays bounded for any n_fits.
 * TLS_E_ARG, before any device work and with the outputs untouched, for n_global or n_local outside
 * [2, TLS_VIEWS_MAX_BINS], a local_durations or local_width that is not finite and > 0, local_width > 2 * local_durations,
 * a curve[f] outside [0, n_curves), n outside [1, 2^20], negative counts, and a t that is not finite and non-decreasing.
 * y is taken as it is (finite); period, T0, duration and secondary_phase may hold any value. */
int tls_folded_views(tls_ctx *ctx, const double *t, const double *y, int64_t n, int64_t n_curves, const double *period,
                     const double *T0, const double *duration, const double *secondary_phase, const int64_t *curve,
                     int64_t n_fits, int64_t n_global, int64_t n_local, double local_durations, double local_width,
                     tls_views_record *out /* [n_fits] */, double *global_median, int32_t *global_count,
                     double *local_median, int32_t *local_count);

/* The variability periodogram: the generalised (floating-mean, weighted) Lomb-Scargle periodogram of Zechmeister & Kuerster
 * (2009, A&A 496, 577) of every curve of a batch on shared time stamps, and the sine test of a candidate.  Is the STAR
 * periodic, and is a candidate just that variability?  For a curve y [n] (weights from dy [n], or uniform) over the ascending
 * t [n], with t_0 = t[0]:
 *   prologue, every sum in index order:
 *       v_i = 1.0 / (dy_i * dy_i);  W = sum v_i;  w_i = v_i / W                   (without dy: w_i = 1.0 / n)
 *       ybar = sum (w_i * y_i);  d_i = y_i - ybar;  a_i = w_i * d_i;  YY = sum (a_i * d_i)
 *   phase of (frequency f, point i):  e = t_i - t_0;  x = f * e;  r = x - floor(x);  phi = 6.283185307179586 * r
 *   six sums:  YC, YS = sum a_i cos phi, sum a_i sin phi;  C, S = sum w_i cos phi, sum w_i sin phi;  C2, S2 = the same two
 *   of w at the frequency 2.0 * f.  They are a dense product -- the rows times one [n x 2 F] matrix that is generated on
 *   the fly -- in fp64 FMAs, i ascending: equal to the exact sums within
 *       (n + 2 pi max|f (t - t_0)| + 8) * 2^-52 * sum_i |A[r][i]|                 (A = a or w)
 *   epilogue, one IEEE double operation a step:
 *       CC = 0.5 * (1.0 + C2) - C * C;  SS = 0.5 * (1.0 - C2) - S * S;  CS = 0.5 * S2 - C * S;  D = CC * SS - CS * CS
 *       power = (SS * YC * YC + CC * YS * YS - 2.0 * CS * YC * YS) / (YY * D)
 *       ca = (YC * SS - YS * CS) / D;  sa = (YS * CC - YC * CS) / D
 *       amplitude = sqrt(ca * ca + sa * sa);  phase = atan2(sa, ca) / 6.283185307179586       (cycles, at t_0)
 *       NaN in all three where D <= 0 or YY <= 0.
 * The prologue equals tests/gls_spec.py bit for bit, and power and amplitude equal its epilogue of the device's own sums bit
 * for bit; phase comes from the device's atan2, which agrees with the host's within a few ulp, not bit for bit. */
#define TLS_GLS_MAX_POINTS (1 << 22)
#define TLS_GLS_MAX_FREQUENCIES (1 << 24)
#define TLS_SINE_MAX_HARMONICS 8

/* The non-uniform DFT of a row matrix: out[r][k] = (sum_i rows[r][i] cos phi_ki, sum_i rows[r][i] sin phi_ki) with phi as
 * above, rows [n_rows][n], any frequencies [n_freq] (not assumed uniform), out [n_rows][n_freq][2].  Needs no plan.
 * n_rows == 0 is a no-op.  TLS_E_ARG, before any device work, for n outside [1, 2^22], n_freq outside [1, 2^24], a t that
 * is not finite and non-decreasing and a frequency that is not finite and > 0. */
int tls_nudft(tls_ctx *ctx, const double *rows, int64_t n_rows, int64_t n, const double *t, const double *frequencies,
              int64_t n_freq, double *out);

/* The periodogram of y [n_curves][n] (dy [n_curves][n], or NULL: uniform weights) at frequencies [n_freq]: out_mean (ybar)
 * and out_variance (YY) [n_curves]; out_power, out_amplitude, out_phase [n_curves][n_freq], each may be NULL.  k > 0 selects
 * the k highest peaks of every curve's power on the device, where it lies, by the selection of tls_find_peaks with
 * periods = 1.0 / frequencies, min_separation and the ratios (0.5, 2.0): out_peaks [n_curves][k], out_n_peaks [n_curves]
 * (chi2, depth NaN and row -1: they have no source); k == 0 selects none.  For tests and tools: out_rows [n_curves][n] (a),
 * out_weights ([n_curves][n] with dy, [n] without) and out_sums [n_curves][n_freq][6] (YC, YS, C, S, C2, S2), each may be
 * NULL.  Curves are processed in slabs, so device memory stays bounded.  TLS_E_ARG as tls_nudft, for n < 3, and for a peaks
 * request tls_find_peaks refuses.  y and dy are taken as they are (finite, dy > 0). */
int tls_lomb_scargle(tls_ctx *ctx, const double *t, const double *y, const double *dy, int64_t n, int64_t n_curves,
                     const double *frequencies, int64_t n_freq, double *out_mean, double *out_variance, double *out_power,
                     double *out_amplitude, double *out_phase, int64_t k, double min_separation, tls_peak *out_peaks,
                     int64_t *out_n_peaks, double *out_rows, double *out_weights, double *out_sums);

/* The sine test of a candidate, after the SWEET test of the Kepler Robovetter: the periodogram's statistic of ONE curve at the
 * periods h * P of a few harmonics h, on the out-of-transit baseline.  Candidate f is (period[f], T0[f], duration[f] in days)
 * on curve curve[f]; T0 and duration may both be NULL (no mask).
 *   status 1 (NaN elsewhere) unless P is finite and > 0 and, with a mask, T0 is finite and d is finite and > 0
 *   with a mask, hw = 0.5 * mask * d:  x = (t_i - T0) / P;  k = floor(x + 0.5);  tau = (x - k) * P;  out iff fabs(tau) <= hw
 *   n_used = the points left;  status 2 (n_used reported, NaN elsewhere) if n_used < 4
 *   an ordered sum of terms q_i: lane j = i mod 256 adds q_i (0.0 for a point that is out) over its i ascending, starting from
 *   0.0; the sum is lane 0's plus lane 1's ... plus lane 255's, in that order
 *   the prologue over the points left with ordered sums (without dy: w_i = 1.0 / n_used); for every harmonic Ph = h * P,
 *   f = 1.0 / Ph, f2 = 2.0 * f, the six sums as ordered sums of the rounded products a_i cos phi, ..., and the epilogue
 *   amplitude_err = sqrt(2.0 * YY * (1.0 - power) / (n_used - 3.0));  significance = amplitude / amplitude_err
 * n_used, mean and variance equal tests/gls_spec.py bit for bit, the sums lie within the bound above, and the harmonic
 * records equal the statement's epilogue of the device's own sums.  All fields are doubles. */
typedef struct tls_sine_record {
    double status;                 /* 0 done; 1 no such candidate / non-finite inputs; 2 fewer than 4 points left */
    double n_used;
    double mean, variance;         /* ybar and YY of the points left */
} tls_sine_record;
typedef struct tls_sine_harmonic {
    double power, amplitude, phase;
    double amplitude_err, significance;
} tls_sine_harmonic;
/* n_fits candidates on the curves of y (dy, or NULL) [n_curves][n] over t [n]; harmonics [n_harmonics] finite and > 0, at
 * most TLS_SINE_MAX_HARMONICS; mask finite and >= 0.  out [n_fits], out_harmonics [n_fits][n_harmonics], out_sums
 * [n_fits][n_harmonics][6] or NULL.  Needs no plan; n_fits == 0 is a no-op; candidates are processed in slabs.  TLS_E_ARG,
 * before any device work, for a curve[f] outside [0, n_curves), n outside [1, 2^22], negative counts, a bad harmonic or
 * mask, one of T0 and duration without the other, and a t that is not finite and non-decreasing. */
int tls_sine_test(tls_ctx *ctx, const double *t, const double *y, const double *dy, int64_t n, int64_t n_curves,
                  const double *period, const double *T0, const double *duration, const int64_t *curve, int64_t n_fits,
                  const double *harmonics, int64_t n_harmonics, double mask, tls_sine_record *out,
                  tls_sine_harmonic *out_harmonics, double *out_sums);

/* Iterative sinusoid pre-whitening: the variability of a star that is FASTER than a transit -- pulsations, a contact binary next
 * door, rapid rotation -- measured by the periodogram above and removed term by term, where no median or biweight window can
 * follow it without flattening the transit too (the harmonic remover of the Kepler TPS, Period04).  For a curve y [n] (weights
 * from dy [n], or uniform) over t [n] and the grid frequencies [n_freq]; r starts as y and trend as 0.0.  Iteration
 * j = 0 .. n_terms - 1, while the curve runs:
 *   spectrum: the periodogram of r on the grid as tls_lomb_scargle forms it (the prologue in index order, the dense product,
 *       the epilogue).  C, S, C2, S2 depend on the weights alone and are formed once a call.  ybar_0 = the mean of the first
 *       prologue.
 *   pick: k = the first index of the largest finite power.  None (a constant row): status 2, the curve stops.
 *       power[k] < min_power: status 1, the curve stops.  The row of a curve that stopped is final.
 *   refine: if 0 < k < n_freq - 1, both neighbours are finite and den = p[k-1] - 2.0 * p[k] + p[k+1] < 0:
 *       half = 0.5 * (f[k+1] - f[k-1]);  f* = f[k] + 0.5 * half * (p[k-1] - p[k+1]) / den;      otherwise f* = f[k]
 *   fit and subtract, for h = 1 .. n_harmonics in turn, each on the row the harmonic before left:  fh = h * f*; the statement
 *       of tls_sine_test without a mask at the frequencies fh and 2.0 * fh (ordered 256-lane sums: W, ybar, YY, then the six
 *       sums of the rounded products, then the epilogue with ca and sa).  A NaN epilogue: the harmonic is skipped, term status
 *       1.  Otherwise, for every i:  u = cos phi_i - C;  v = sin phi_i - S;  q = ca * u + sa * v;  r_i = r_i - q;
 *       trend_i = trend_i + q
 * At the end trend_i = ybar_0 + trend_i and flat_i = y_i / trend_i: the variability multiplies the transit, and the other
 * detrenders return flat = y / trend too.  Every step is one IEEE double operation, contraction off.  The means and variances
 * equal tests/prewhiten_spec.py bit for bit, the six sums lie within the periodogram's bound, the pick equals the statement's
 * wherever its highest power stands clear of the others, f*, ca, sa, power and amplitude equal the statement's steps on the
 * device's own powers and sums bit for bit, and a subtraction differs from the statement's by the few ulp of the device's
 * cos and sin.  A term fitted near a transit's period or one of its harmonics removes part of the transit: min_power and the
 * frequency grid are the caller's protection (DESIGN.md "Pre-whitening").  All fields are doubles.  16 doubles. */
#define TLS_PREWHITEN_MAX_TERMS 32
#define TLS_PREWHITEN_LDS_POINTS 6144   /* rows of at most this many points are fitted in the LDS, longer ones in device memory */
typedef struct tls_prewhiten_term {
    double status;                 /* 0 fitted and subtracted; 1 the epilogue was NaN, nothing subtracted; 2 not reached */
    double index, frequency_grid;  /* k and f[k] of the pick */
    double power_left, power_peak, power_right;   /* p[k-1], p[k], p[k+1]; NaN where the grid ends */
    double frequency;              /* h * f* */
    double mean, variance;         /* ybar and YY of the row fitted (ordered 256-lane sums) */
    double ca, sa, C, S;
    double power, amplitude, phase;   /* at `frequency`, of the row fitted */
} tls_prewhiten_term;
/* y (dy, or NULL: uniform weights) [n_curves][n] over t [n]; n_terms in [1, TLS_PREWHITEN_MAX_TERMS], n_harmonics in
 * [1, TLS_SINE_MAX_HARMONICS], min_power in [0, 1].  out_flat [n_curves][n]; out_trend the same or NULL; out_terms
 * [n_curves][n_terms][n_harmonics]; out_n_iterations [n_curves]: the iterations that fitted; out_status [n_curves]: 0 every
 * iteration ran, 1 stopped below min_power, 2 stopped without a finite power.  For tests: out_steps
 * [n_terms * n_harmonics + 1][n_curves][n], the row entering every (iteration, harmonic) and, last, the final row (a step
 * that was not reached holds the final row), or NULL; out_sums [n_curves][n_terms][n_harmonics][6] (YC, YS, C, S, C2, S2) or
 * NULL.  The rows stay on the device for the whole call; the host reads one count an iteration and stops when no curve
 * runs.  Curves are processed in slabs, so device memory stays bounded.  Needs no plan.  n_curves == 0 is a no-op.
 * TLS_E_ARG, before any device work, as tls_lomb_scargle, and for n_terms, n_harmonics or min_power out of range.  y and dy
 * are taken as they are (finite, dy > 0). */
int tls_prewhiten(tls_ctx *ctx, const double *t, const double *y, const double *dy, int64_t n, int64_t n_curves,
                  const double *frequencies, int64_t n_freq, int64_t n_terms, int64_t n_harmonics, double min_power,
                  double *out_flat, double *out_trend, tls_prewhiten_term *out_terms, int64_t *out_n_iterations,
                  double *out_status, double *out_steps, double *out_sums);
/* Pre-whitening that cannot see the transit: tls_prewhiten with other weights and nothing else changed.  mask [n_curves][n],
 * != 0: protected.  v_i = 0.0 at a protected point and 1.0 / (dy_i * dy_i) or, without dy, 1.0 elsewhere; W = the ordered sum of
 * the v_i (in index order in the periodogram's prologue, over 256 lanes in the fit) and w_i = v_i / W.  Mean, variance,
 * periodogram, pick, refinement and sinusoid fit use these weights (every curve has a weight row of its own, as with a dy);
 * the subtraction and the trend cover EVERY point, the protected ones included.  A row with fewer than 3 unprotected points
 * has nothing removed: status 2, n_iterations 0, trend = its mean with the mask ignored.  An all-zero mask has the weights of
 * tls_prewhiten (without dy, W is the sum of n ones, so 1.0 / W is 1.0 / n); without dy the sums of the weights then come from
 * one dense product a curve instead of one a call, which may move the last bits.  Everything else, the errors included, as
 * tls_prewhiten. */
int tls_prewhiten_masked(tls_ctx *ctx, const double *t, const double *y, const double *dy, const uint8_t *mask, int64_t n,
                         int64_t n_curves, const double *frequencies, int64_t n_freq, int64_t n_terms, int64_t n_harmonics,
                         double min_power, double *out_flat, double *out_trend, tls_prewhiten_term *out_terms,
                         int64_t *out_n_iterations, double *out_status, double *out_steps, double *out_sums);

/* ---- survey mode: the ephemeris match across the candidates of a batch ----------------------------------------------- */
/* The test that looks across the stars (Coughlin et al. 2014): the stars of one field, camera and sector contaminate one
 * another and share instrumental periods.  A faint star next to an eclipsing binary shows the binary's period and epoch at a
 * diluted depth and passes every single-curve test, because the signal in its light curve is real.  Candidates on different
 * stars that share a period (or an integer multiple of it) and an epoch are flagged, the strongest is taken as the source,
 * and a period that many stars show with no common epoch is a systematic: that count is reported too.
 * Candidate f is (star[f], any int64; period[f], T0[f], duration[f] in days; strength[f], larger = more likely the source).
 * It is GOOD when period, T0, duration and strength are finite, period > 0 and duration > 0.  A bad candidate gets status 1
 * and NaN in every other field, and is invisible to every other candidate.  For a good f and every good g != f with
 * star[g] != star[f], with (l, s) = the member of the longer / the shorter period (equal periods: either gives the same bits):
 *   m = rint(P_l / P_s)  (half to even);  e = m * P_s;  dP = fabs(P_l - e);  c = span / P_l;  drift = dP * c
 *   dmax = fmax(d_f, d_g);  plim = drift_tolerance * dmax;  elim = epoch_tolerance * dmax
 *   period_match = (m <= max_ratio) and (drift <= plim)
 *   x = (T0_l - T0_s) / P_s;  r = rint(x);  u = x - r;  dt = fabs(u) * P_s
 *   match = period_match and (dt <= elim)
 * Both relations are symmetric in (f, g) bit for bit.  drift is how far the two ephemerides slide apart over the span, dt
 * the distance of the epochs modulo the shorter period.  The record of f:
 *   n_same = the g with period_match and m == 1 (the pile-up count);  n_period = the g with period_match;  n_match = the g
 *   with match;  best = the index g of the match of the largest strength, the lowest index among equals, -1 without one;
 *   best_ratio = +m if P_best >= P_f, else -m;  best_dt, best_drift = that pair's dt and drift;  best_strength =
 *   strength[best];  child = 1 if strength[best] > strength[f], else 0;  the last five NaN without a match.
 * Every step is one IEEE double operation, counts and an argmax with the lowest index do not depend on the order of
 * evaluation, and no sum of doubles occurs: the record equals the numpy statement in tests/ephemeris_match_spec.py bit for
 * bit.  Counts and indices are doubles.  10 doubles. */
#define TLS_MATCH_MAX_CANDIDATES 1048576
#define TLS_MATCH_MAX_RATIO 64
typedef struct tls_match_record {
    double status;                 /* 0 matched against the others; 1 a bad candidate */
    double n_same, n_period, n_match;
    double best, best_ratio, best_dt, best_drift, best_strength;
    double child;
} tls_match_record;
/* The records of n candidates; out [n].  Needs no plan and no search, and leaves a prepared plan as it is.  TLS_E_ARG, before
 * any device work, unless span is finite and > 0, both tolerances are finite and >= 0, max_ratio is in [1, 64] and
 * n is in [0, 2^20].  n == 0 is a no-op.  All pairs are tested: the work grows with n * n. */
int tls_ephemeris_match(tls_ctx *ctx, const int64_t *star, const double *period, const double *T0, const double *duration,
                        const double *strength, int64_t n, double span, double drift_tolerance, double epoch_tolerance,
                        int64_t max_ratio, tls_match_record *out);

/* ---- survey mode: the per-star noise profile (a robust CDPP by window width) ------------------------------------------- */
/* How noisy is each star on the time scale of a transit?  For every curve y [n] (a -0.0 is taken as +0.0) over the shared time
 * stamps t [n] (or NULL: no gaps), with K = 1.4826022185056018 and median(v [m]) = the value of rank m / 2 of the sorted
 * values for odd m, 0.5 * (s[m/2 - 1] + s[m/2]) for even m:
 *   m = median(y);  d_j = y_j - m;  sigma = K * median(|d_j|)
 *   sigma == 0: status 1, n_clipped 0, n_pairs 0, sigma_p2p NaN, every per-width value NaN, every count 0
 *   keep_j = (d_j <= clip_upper * sigma) and (d_j >= -(clip_lower * sigma));  n_clipped = the others.  One pass, internal to
 *   the measurement; an infinite clip switches its side off
 *   pairs = the j with keep_j, keep_{j+1} and t_{j+1} - t_j <= pair_span;  n_pairs their number
 *   sigma_p2p = (K * median(|y_{j+1} - y_j| over the pairs)) / 1.4142135623730951, NaN without a pair
 * and for every width w = widths[k] (samples), window i = the samples [i, i + w), i = 0 .. n - w:
 *   valid_i = every sample kept and t[i + w - 1] - t[i] <= span_max[k]
 *   v_i = (((0.0 + d_i) + d_{i+1}) + ... + d_{i+w-1}) / w          (the direct sum, left to right: no prefix sums)
 *   count = the valid windows;  count < min_count: robust and rms NaN
 *   mu = median(valid v);  robust = K * median(|v_i - mu| over the valid)
 *   mean = lanes(v) / count;  rms = sqrt(lanes((v_i - mean) * (v_i - mean)) / count)
 * lanes() is the sine test's ordered sum over 256 lanes (window i on lane i mod 256).  Every step is one IEEE double
 * operation and every median a selection, so the results equal the numpy statement in tests/noise_profile_spec.py bit for
 * bit.  The caller forms span_max[k] = (w - 1 + gap_tolerance) * cadence and pair_span = (1 + gap_tolerance) * cadence.
 * Counts in the record are doubles.  6 doubles. */
#define TLS_NOISE_MAX_WIDTH 4096
#define TLS_NOISE_MAX_WIDTHS 64
#define TLS_NOISE_MAX_POINTS 4194304
#define TLS_NOISE_LDS_POINTS 8192   /* rows of at most this many points are measured in the LDS, longer ones in device memory */
typedef struct tls_noise_curve {
    double status;                 /* 0 measured; 1 sigma == 0 (a constant row, or more than half of it on one value) */
    double n_clipped, n_pairs;
    double median, sigma, sigma_p2p;
} tls_noise_curve;
/* The profiles of n_curves rows; out_curves [n_curves], out_count, out_robust, out_rms [n_curves][n_widths].  Needs no plan
 * and no search, and leaves a prepared plan as it is.  Curves are processed in slabs, so device memory stays bounded.
 * n_curves == 0 is a no-op.  TLS_E_ARG, before any device work, unless n is in [3, TLS_NOISE_MAX_POINTS], n_widths in
 * [1, TLS_NOISE_MAX_WIDTHS], the widths strictly ascending in [1, min(n, TLS_NOISE_MAX_WIDTH)], every span_max and
 * pair_span >= 0 (inf allowed), both clips >= 0 (inf allowed), min_count >= 1, y finite and t (where given) finite and
 * ascending. */
int tls_noise_profile(tls_ctx *ctx, const double *t, const double *y, int64_t n, int64_t n_curves, const int64_t *widths,
                      const double *span_max, int64_t n_widths, double pair_span, double clip_upper, double clip_lower,
                      int64_t min_count, tls_noise_curve *out_curves, int64_t *out_count, double *out_robust, double *out_rms);

/* ---- survey mode: regression detrending against centroids and basis vectors -------------------------------------------- */
/* A weighted, robust linear least-squares fit of every light curve against series that are known to drive its systematics: the
 * columns shared [n_shared][n] every curve takes (cotrending basis vectors, SysRem profiles of another ensemble) and then the
 * columns own [n_curves][n_own][n] of the curve itself (monomials of its centroids); m = n_shared + n_own in
 * [1, TLS_DECOR_MAX_TERMS]; the mean is always free.  y [n_curves][n]; dy (or NULL) gives w = 1.0 / (dy * dy), else w = 1.0;
 * mask (or NULL) [n_curves][n], != 0: protected.  segments [n_segments + 1] ascends strictly from 0 to n; every
 * (curve, segment) is fitted on its own.  F starts as the unprotected points of the segment; clip rounds run = 0.  Every sum
 * runs over the points of F in ascending index from +0.0:
 *   fit:
 *     A  W = sum w * 1.0;  Sy = sum w * y;  Sk = sum w * x_k;  mu = Sy / W;  mean_k = Sk / W
 *        F empty: status 1 with these sums over the whole segment
 *     B  d = x_k - mean_k;  Vk = sum (w * d) * d;  scale_k = sqrt(Vk / W)
 *        column k is live if 0 < scale_k < inf, else dropped (bit k of `dropped`)
 *        |F| < live + 2: status 1
 *     C  z = y / mu - 1.0;  u_k = (x_k - mean_k) / scale_k (live), 0.0 (dropped)
 *        G_kl = sum (w * u_k) * u_l for l <= k;  G_kk = G_kk + ridge * W;  b_k = sum (w * u_k) * z
 *     D  Cholesky in place, j ascending over the live columns:
 *            s = G_jj;  for k < j live, ascending:  s = s - L_jk * L_jk
 *            not (s > TLS_DECOR_PIVOT * G_jj): column j is collinear with those before it: dropped (bit j), no longer live
 *            L_jj = sqrt(s);  for i > j live, ascending:  q = G_ij;  for k < j live, ascending:  q = q - L_ik * L_jk;  L_ij = q / L_jj
 *        forward, j ascending live:  s = b_j;  for k < j live, ascending:  s = s - L_jk * v_k;  v_j = s / L_jj
 *        back, j descending live:    s = v_j;  for k > j live, ascending:  s = s - L_kj * c_k;  c_j = s / L_jj
 *        c_k = 0.0 for a dropped column
 *     E  p = 0.0;  for k live, ascending:  p = p + c_k * u_k;  r = z - p  (every point of the segment)
 *        Q = sum (w * r) * r;  sigma = sqrt(Q / W)
 *   clip, only while rounds < n_iter:  up = sigma_upper * sigma;  down = -(sigma_lower * sigma)
 *        a member of F leaves if r > up or r < down (inf switches a side off);  rounds = rounds + 1;  if any left: fit again
 *   status 1 (at any fit): every c_k = 0.0, no column live or dropped, mean_k = 0.0, scale_k = 1.0, sigma = NaN
 *   trend = mu * (1.0 + p);  flat = y / trend at EVERY point of the segment, protected and clipped ones included
 *   status 2 (a trend value of the segment is not finite or not > 0): trend = mu, flat = y / mu; the rest of the record stays
 * Every step is one IEEE double operation, so the results equal the Python statement in tests/decorrelate_spec.py bit for bit.
 * A mask of zeros gives the bits of a call without one.  coef / scale are the coefficients in the units of the raw columns. */
#define TLS_DECOR_MAX_TERMS 16
#define TLS_DECOR_MAX_ITER 16
#define TLS_DECOR_PIVOT 1e-10
#define TLS_DECOR_LDS_POINTS 32768   /* a segment of at most this many points keeps F in the LDS, a longer one in device memory */
typedef struct tls_decor_fit {
    double status;                 /* 0 fitted; 1 too few points; 2 fitted, but the trend left (0, inf): trend = mu */
    double dropped;                /* bit k: column k is constant on F or collinear with the columns before it */
    double n_fit, n_clipped;       /* |F| at the end; the points the clip removed */
    double rounds;                 /* clip rounds run */
    double mu, sigma;
    double n_live;                 /* the columns of the final fit */
} tls_decor_fit;
/* out_flat, out_trend (may be NULL) [n_curves][n]; out_fit [n_curves][n_segments]; out_coef, out_mean, out_scale (each may be
 * NULL) [n_curves][n_segments][m].  The shared columns go to the device once a call; curves are processed in slabs, so device
 * memory stays bounded.  Needs no plan and no search, and leaves a prepared plan as it is.  n_curves == 0 is a no-op.
 * TLS_E_ARG, before any device work and with the outputs untouched, unless n is in [1, 1e8], m in [1, TLS_DECOR_MAX_TERMS],
 * n_segments in [1, n] with segments ascending strictly from 0 to n, ridge finite and >= 0, n_iter in [0, TLS_DECOR_MAX_ITER],
 * both sigmas > 0 (inf allowed, no NaN), y and dy finite and > 0, and every column finite. */
int tls_decorrelate(tls_ctx *ctx, const double *y, const double *dy, const uint8_t *mask, int64_t n, int64_t n_curves,
                    const double *shared, int64_t n_shared, const double *own, int64_t n_own, const int64_t *segments,
                    int64_t n_segments, double ridge, int64_t n_iter, double sigma_upper, double sigma_lower, double *out_flat,
                    double *out_trend, tls_decor_fit *out_fit, double *out_coef, double *out_mean, double *out_scale);

/* ---- survey mode: robust B-spline detrending with a BIC-chosen knot spacing ------------------------------------------------ */
/* Penalised least squares on a uniform cubic B-spline in every gap-free segment of the shared time stamps t [n] (finite,
 * non-decreasing), with iterative sigma clipping of the residuals and, where several knot spacings are given, the spacing of
 * the least Bayesian information criterion for every curve: the "Kepler spline" of Vanderburg & Johnson (2014).  y [n_rows][n];
 * dy (or NULL) gives w = 1.0 / (dy * dy), else w = 1.0; mask (or NULL) [n_rows][n], != 0: protected, never a member of a fit.
 * A new segment starts behind every gap t[j] - t[j-1] > break_tolerance.  A (curve, segment, spacing) with the points a .. b,
 * L of them, T = t[b] - t[a]:
 *   knots   T == 0: q = 0, m = 0, status 1.  Else q = max(1, ceil(T / spacing)), h = T / q, m = q + 3 coefficients.
 *   place   x = (t[i] - t[a]) / h;  j = min(int(x), q - 1);  u = x - j            (the last point: u = 1 in the last interval)
 *   basis   u2 = u * u;  u3 = u2 * u;  o = 1.0 - u;  o2 = o * o;  o3 = o2 * o
 *           b0 = o3 / 6.0;  b1 = ((3.0 * u3 - 6.0 * u2) + 4.0) / 6.0;  b2 = (((-(3.0 * u3) + 3.0 * u2) + 3.0 * u) + 1.0) / 6.0
 *           b3 = u3 / 6.0;  point i touches the coefficients j .. j + 3
 *   F       the members: at first the unprotected points;  rounds = dropped = 0;  sigma = NaN
 *   fit:    nF = |F|;  nF == 0, or the last member's time stamp is not > the first one's: status 1, leave the loop
 *      A    W = sum_F w in index order from +0.0
 *           interval j, its members (a contiguous index range, t ascends) in ascending index, every sum from +0.0:
 *               wb_k = w * b_k;  S_j[k][l] += wb_k * b_l  (k <= l, ten sums);  R_j[k] += wb_k * y  (four)
 *           A[c][c + d] (d = 0 .. 3, c + d < m) = 0.0 + the S_j[c - j][c + d - j] of j = max(0, c + d - 3) .. min(c, q - 1), ascending
 *           g[c] = 0.0 + the R_j[c - j] of j = max(0, c - 3) .. min(c, q - 1), ascending
 *           pw = W / q;  lam = penalty * pw;  A[c][c + d] = A[c][c + d] + lam * P[c][c + d], d = 0 .. 2, P = D2^T D2 of the
 *           second differences of the m coefficients (whole numbers): positive definite with penalty > 0 as soon as F holds two
 *           distinct time stamps, whatever intervals are empty
 *      B    Cholesky inside the band, j ascending:  s = A[j][j];  for k = max(0, j - 3) .. j - 1:  s = s - L[j][k] * L[j][k]
 *               not (s > TLS_SPLINE_PIVOT * A[j][j]): status 2, leave the loop;  L[j][j] = sqrt(s)
 *               for i = j + 1 .. min(j + 3, m - 1):  v = A[j][i];  for k = max(0, i - 3) .. j - 1:  v = v - L[i][k] * L[j][k]
 *                   L[i][j] = v / L[j][j]
 *           forward, j ascending:  s = g[j];  for k = max(0, j - 3) .. j - 1:  s = s - L[j][k] * z[k];  z[j] = s / L[j][j]
 *           back, j descending:    s = z[j];  for k = j + 1 .. min(j + 3, m - 1):  s = s - L[k][j] * c[k];  c[j] = s / L[j][j]
 *      C    trend at EVERY point:  p = c[j] * b0;  p = p + c[j+1] * b1;  p = p + c[j+2] * b2;  p = p + c[j+3] * b3
 *           a value not in (0, inf): status 2, leave the loop;  else status 0
 *   clip    rounds == n_iter: leave.  r = y - trend over F;  med = median(r);  sigma = 1.4826 * median(|r - med|), the median
 *           of an even count being (lower + upper) / 2;  sigma == 0: leave
 *           up = sigma_upper * sigma;  down = -(sigma_lower * sigma);  out: the members with r > up or r < down
 *           rounds = rounds + 1;  nobody out: leave;  nF - |out| < 2: leave, the round is not applied
 *           F = F without out;  dropped = dropped + |out|;  fit again
 *   status 1, 2:  trend = (sum w * y) / (sum w) over F in index order, over all the points of the segment where F is empty
 *   flat = y / trend at every point;  weight = sum_F w (0.0: no member);  r = y - trend;  ssr = sum_F (w * r) * r
 * The choice, for every curve (one spacing: the same record, choice 0):
 *   d = y[i+1] - y[i] of the neighbours of one segment that are both unprotected; none: sigma_pp = NaN
 *   sigma_pp = (1.4826 * median(|d - median(d)|)) / sqrt(2)
 *   spacing s over its segments of status 0, in order, from 0:  K = sum coefficients;  N = sum kept;  Q = sum ssr;  V = sum weight
 *   bic[s] = K * log(N) + (Q / (V / N)) / (sigma_pp * sigma_pp);  the first index of the least finite one wins
 *   sigma_pp not > 0, or no bic finite: the first spacing, flag = 1
 * Every step but log is one IEEE double operation without contraction, so flat, trend and the segment records equal the Python
 * statement in tests/spline_spec.py bit for bit, and bic within the ulp of log.  One spacing gives the bits of that spacing in
 * a list in which it wins; a mask of zeros gives the bits of a call without one. */
#define TLS_SPLINE_MAX_SPACINGS 16
#define TLS_SPLINE_MAX_ITER 16
#define TLS_SPLINE_MAX_COEF 512      /* the most coefficients of one segment: the band the LDS holds */
#define TLS_SPLINE_LDS_POINTS 5120   /* a call whose longest segment has at most this many points keeps the segment in the LDS */
#define TLS_SPLINE_PIVOT 1e-10
typedef struct tls_spline_segment {
    double status;                 /* 0 fitted; 1 fewer than two members with distinct time stamps; 2 a pivot failed or the
                                      trend left (0, inf): for 1 and 2 the trend is the weighted mean */
    double intervals, coefficients;/* q and m (0: T == 0) */
    double points, kept;           /* L, and |F| at the end */
    double rounds, dropped;        /* clip rounds run, points they removed */
    double sigma;                  /* of the last round (NaN: none) */
    double ssr, weight;            /* sum_F (w r) r, sum_F w */
} tls_spline_segment;
typedef struct tls_spline_curve {
    double choice;                 /* index of the chosen spacing */
    double sigma_pp;
    double flag;                   /* 1: no BIC could be formed, the first spacing was taken */
    double bic[TLS_SPLINE_MAX_SPACINGS];   /* NaN behind n_spacings */
} tls_spline_curve;
/* out_flat, out_trend (may be NULL) [n_rows][n]; out_segment_records [n_rows][n_segments] for the segments of t in order;
 * out_curve_records [n_rows].  Needs no plan and no search, and leaves a prepared plan as it is.  n_rows == 0 is a no-op.
 * TLS_E_ARG, before any device work and with the outputs untouched, unless n is in [1, 1e8], t is finite and non-decreasing,
 * n_spacings is in [1, TLS_SPLINE_MAX_SPACINGS] with every spacing finite and > 0, break_tolerance > 0 (inf allowed), penalty
 * finite and >= 0, n_iter in [0, TLS_SPLINE_MAX_ITER], both sigmas > 0 (inf allowed, no NaN), y and dy finite and > 0, and no
 * segment at any spacing has more than TLS_SPLINE_MAX_COEF coefficients. */
int tls_spline_detrend(tls_ctx *ctx, const double *t, const double *y, const double *dy, const uint8_t *mask, int64_t n,
                       int64_t n_rows, const double *spacings, int64_t n_spacings, double break_tolerance, double penalty,
                       int64_t n_iter, double sigma_upper, double sigma_lower, double *out_flat, double *out_trend,
                       tls_spline_segment *out_segment_records, tls_spline_curve *out_curve_records);

/* ---- survey mode: missing points and outliers flagged and repaired -------------------------------------------------------- */
/* The cleaning stage in front of every other one: the bad points of every curve are flagged and replaced with defined values,
 * so that a batch whose stars have their own missing cadences, flares and single-sample glitches keeps its shared time stamps.
 * t [n] finite and non-decreasing; y [n_rows][n] MAY hold NaN, +-inf, zero and negative values; bad (or NULL) [n_rows][n],
 * != 0: the caller's quality flag.  window_length > 0 in days gives a sliding centre, 0.0 the row's median.
 *   flags   uint8 a point: 1 missing, not (isfinite(y) and y > 0); 2 the caller's bad; 4 high outlier; 8 low outlier.  A point
 *           is valid while its flags are 0.
 *   windows the biweight's: a new segment starts behind every gap t[j] - t[j-1] > break_tolerance; the window of i is the
 *           points of its segment with |t[j] - t[i]| <= 0.5 * window_length (at most TLS_BIWEIGHT_MAX_WINDOW).
 *   median  the middle value, or (a + b) / 2.0 of the two middle ones.
 *   round   up to n_iter of them, none when both sigmas are inf:
 *     1  window_length 0: centre = median of the row's valid points, every valid point has a residual.  Else the centre of a
 *        valid point is the median of the valid points of its window OTHER THAN ITSELF; with fewer than min_points of those
 *        the point has no residual this round and the clip cannot flag it.
 *     2  r_i = y_i - centre_i
 *     3  fewer than two points with a residual: the rounds end, this one is not counted.  Over the points with a residual:
 *        c0 = median(r);  sigma = 1.4826 * median(|r_i - c0|);  rounds = rounds + 1;  the record's center = the row's median
 *        (window_length 0) or c0, its sigma = sigma
 *     4  not (sigma > 0): the rounds end
 *     5  d_i = r_i - c0;  high: d_i > sigma_upper * sigma;  low candidate: d_i < -(sigma_lower * sigma)
 *     6  a run: a maximal set of low candidates that are neighbours in the sequence of the round's valid points of one
 *        segment -- an invalid point is stepped over; a valid point that is no candidate (without a residual, high) and a
 *        segment boundary end a run.  The candidates of a run of at most max_run are flagged low: a transit, a run of many
 *        samples, is left alone, and a missing sample inside it does not split it.
 *     7  nobody flagged: the rounds end.  Fewer than two valid points would be left: the round is not applied, the rounds end.
 *        Else flags |= 4 (high), |= 8 (low).
 *   repair  a point with flags != 0, a < i < b its nearest valid points inside its segment:
 *           both: y_a where t_b == t_a, else y_a + (y_b - y_a) * ((t_i - t_a) / (t_b - t_a));  one: that neighbour's value;
 *           none: the median of the row's valid points (status |= 1);  a row without a valid point: all 1.0 (status = 2)
 * Valid points pass through with their bits; the output is finite and > 0.  Every step is one IEEE double operation without
 * contraction and the medians are selections, so rows, flags and records equal the Python statement in tests/clean_spec.py
 * bit for bit.  bad of zeros gives the bits of no bad. */
#define TLS_CLEAN_MAX_ITER 16
#define TLS_CLEAN_LDS_POINTS 8192    /* a row of at most this many points keeps a round's residuals in the LDS */
typedef struct tls_clean_record {
    double status;                 /* 0; |= 1 a segment was filled from the row's median; 2 no valid point in the row */
    double n_missing, n_bad;       /* points with flag 1, with flag 2 */
    double n_high, n_low;          /* points with flag 4, with flag 8 */
    double n_filled;               /* points with any flag */
    double longest_run;            /* the longest stretch of consecutive filled indices */
    double rounds;                 /* clip rounds that formed a sigma */
    double center, sigma;          /* of the last such round (NaN: none) */
} tls_clean_record;
/* out_rows [n_rows][n]; out_flags (may be NULL) [n_rows][n]; out_records [n_rows].  Needs no plan and no search, and leaves a
 * prepared plan as it is.  n_rows == 0 is a no-op.  TLS_E_ARG, before any device work and with the outputs untouched, unless n
 * is in [1, 1e8], t is finite and non-decreasing, window_length is finite and >= 0, break_tolerance > 0 (inf allowed), both
 * sigmas > 0 (inf allowed, no NaN), max_run >= 1, n_iter in [0, TLS_CLEAN_MAX_ITER], min_points >= 1 and no window holds more
 * than TLS_BIWEIGHT_MAX_WINDOW points. */
int tls_clean_rows(tls_ctx *ctx, const double *t, const double *y, const uint8_t *bad, int64_t n, int64_t n_rows,
                   double window_length, double break_tolerance, double sigma_upper, double sigma_lower, int64_t max_run,
                   int64_t n_iter, int64_t min_points, double *out_rows, uint8_t *out_flags, tls_clean_record *out_records);

/* The limb-darkened transit fit: the planet's size, impact parameter and T14 from the dip itself, with the exposure time in
 * the model.  A straight chord at constant speed crosses a limb-darkened disc: the separation is z^2 = b^2 + ((1 + k)^2 - b^2)
 * v^2, v = (time from mid-transit) / (T / 2), contacts at |v| == 1; the dip at z comes from a profile table the HOST forms
 * (any limb-darkening law: the device needs no acos and no log), averaged over S sub-exposures; the depth amplitude A is free
 * and the baseline fixed at 1.  For a curve (y [n], dy [n] over the ascending, finite t [n]), a candidate (P, T0, d in days,
 * seed row j0), the table k_rows[nK] ascending and > 0 with profile[nK][M + 1], profile[j][m] = 1 - F((1 + k_rows[j]) m / M;
 * k_rows[j]) and profile[j][M] = 0, the ascending tables impact[nB] in [0, 1) (b as a fraction of 1 + k), ratio[nT] > 0,
 * shift[nS], and the sub-exposure offsets sub[S] in days (S == 1, sub[0] == 0: no smearing):
 *   w = 1.0 / (dy * dy);  xw = (1.0 - y) * w
 *   status 1 and NaN in every other field unless P, T0, d are finite, P > 0, d > 0 and wd = window * d < 0.5 * P
 *   members, i ascending:  x = (t[i] - T0) / P;  k = floor(x + 0.5);  tau = (x - k) * P;  member iff fabs(tau) <= wd
 *   x2 = x2 + (xw * xw) / w over the members in index order
 *   one pass with row j, p = profile[j]:  e1 = 1.0 + k_rows[j];  e2 = e1 * e1;  sM = M / e1
 *     unit (ib, a, c), ib outermost, c innermost (unit index (ib * nT + a) * nS + c):
 *       b = impact[ib] * e1;  bb = b * b;  cc = e2 - bb;  T = d * ratio[a];  rh = 1.0 / (0.5 * T);  c0 = d * shift[c]
 *       cnt = 0; N = 0; D = 0; over the members in index order:
 *         acc = 0.0;  for s = 0 .. S - 1:  ts = tau + sub[s];  v = (ts - c0) * rh;  vv = v * v;  zz = bb + cc * vv
 *           sample = 0.0 unless zz < e2, else  z = sqrt(zz);  q = z * sM;  m = min(floor(q), M - 1);  fr = q - m
 *           sample = p[m] + (p[m + 1] - p[m]) * fr;  acc = acc + sample
 *         mval = acc / S;  the member counts iff mval > 0:  cnt += 1;  N = N + xw * mval;  D = D + w * (mval * mval)
 *       valid iff cnt >= min_count and D > 0 and A = N / D > 0;  q = N / sqrt(D)
 *     the pick = the valid unit of the largest q, the first in unit order among equals
 *   pass 1 uses row j0;  k1 = k_rows[j0] * sqrt(A of its pick);  j1 = the row of the least fabs(k_rows[j] - k1), the lowest j
 *   among equals;  pass 2 uses row j1 (where j1 == j0 it is pass 1);  status 2 (n_points reported, the rest NaN) if a pass
 *   has no valid unit.  The row only shapes ingress and egress; the size is carried by A:  k = k_rows[j1] * sqrt(A).
 *   intervals: the least and the largest k_rows[j1] * sqrt(A_u), b_u, T_u, c0_u over the valid units of pass 2 with
 *   q_u * q_u >= q * q - delta: a profile-likelihood range.
 * Every step is one IEEE double operation and every sum runs in index order: the record equals the Python statement in
 * tests/transit_fit_spec.py bit for bit.  All fields are doubles; `reserved` is 0 whatever the status. */
#define TLS_TRANSIT_FIT_MAX_UNITS 65536
#define TLS_TRANSIT_FIT_MAX_M 4096
#define TLS_TRANSIT_FIT_MAX_SUB 16
#define TLS_TRANSIT_FIT_MAX_ROWS 4096
typedef struct tls_transit_fit_record {
    double status;                 /* 0 fitted; 1 no such candidate (P, T0, d, or a window of half a period or more); 2 no valid unit */
    double n_points;               /* the members */
    double n_in;                   /* cnt of the pick */
    double row_first, row;         /* j0, j1 */
    double ses, amplitude;         /* q and A of the pick */
    double k, b, duration, shift;  /* k_rows[j1] * sqrt(A), impact[ib] * (1 + k_rows[j1]), T (days), c0 (days) */
    double i_impact, i_duration, i_shift;      /* ib, a, c */
    double x2;                     /* sum of (1 - y)^2 / dy^2 over the members */
    double k_lo, k_hi, b_lo, b_hi, duration_lo, duration_hi, shift_lo, shift_hi;
    double reserved;
} tls_transit_fit_record;
/* n_fits candidates (period[f], T0[f], duration[f], row_first[f]) on the curves curve[f] of y, dy [n_curves][n] over the
 * shared time stamps t [n].  out_records [n_fits].  Needs no plan and no search, and leaves a prepared plan as it is.
 * n_fits == 0 is a no-op.  Candidates are processed in slabs, so device memory stays bounded for any n_fits.  TLS_E_ARG,
 * before any device work and with the output untouched, for a curve[f] outside [0, n_curves), a row_first[f] outside
 * [0, n_k), n outside [1, 2^22], negative counts, an empty table, n_b * n_t * n_s above TLS_TRANSIT_FIT_MAX_UNITS, M outside
 * [1, TLS_TRANSIT_FIT_MAX_M], n_sub outside [1, TLS_TRANSIT_FIT_MAX_SUB], n_k above TLS_TRANSIT_FIT_MAX_ROWS, a table that is
 * not finite and non-decreasing (sub and profile: finite), k_rows[0] <= 0, impact outside [0, 1), a ratio <= 0, a window
 * that is not finite or, for a candidate with finite d > 0, has window * d below (0.5 * ratio[n_t-1] + max(fabs(shift[0]),
 * fabs(shift[n_s-1]))) * d + max fabs(sub[s]) (the widest, farthest shifted model plus half an exposure must lie inside the
 * window), min_count < 1, a non-finite or negative delta, and a t that is not finite and non-decreasing.  y and dy are taken
 * as they are (dy > 0); period, T0 and duration may hold any value (status 1). */
int tls_transit_fit(tls_ctx *ctx, const double *t, const double *y, const double *dy, int64_t n, int64_t n_curves,
                    const int64_t *curve, const double *period, const double *T0, const double *duration,
                    const int64_t *row_first, int64_t n_fits, const double *k_rows, const double *profile, int64_t n_k,
                    int64_t M, const double *impact, int64_t n_b, const double *ratio, int64_t n_t, const double *shift,
                    int64_t n_s, const double *sub, int64_t n_sub, double window, int64_t min_count, double delta,
                    tls_transit_fit_record *out_records /* [n_fits] */);

/* The multi-planet search of survey mode: the fitted transits of a batch divided out, so that the next tls_power_batch on
 * the quotient finds the planet under the one found.  The time stamps stay shared -- no point is deleted.  Candidate f
 * (curve[f] in [0, n_curves), or curve NULL: candidate f belongs to curve f) carries period[f] and T0[f] of a peak and
 * row[f], amplitude[f], b[f], duration[f], shift[f] of its tls_transit_fit_record (row, amplitude, b, duration, shift), with
 * the k_rows, profile and sub that fit was made with.  Its constants, one IEEE double operation a step, no contraction:
 *   e1 = 1.0 + k_rows[row];  e2 = e1 * e1;  sM = M / e1;  bb = b * b;  cc = e2 - bb;  rh = 1.0 / (0.5 * duration)
 * It takes part (out_status[f] = 0) iff period, T0, amplitude, b, duration and shift are finite, period > 0, duration > 0,
 * amplitude > 0, b >= 0, bb < e2 and amplitude * (the largest profile[row][m]) < 1.0; any other is skipped (out_status[f] =
 * 1) and changes nothing.  For every point i of a curve, the candidates of that curve that take part in ascending f:
 *   x = (t[i] - T0) / period;  k = floor(x + 0.5);  tau = (x - k) * period
 *   acc = 0.0;  for s = 0 .. S - 1:  ts = tau + sub[s];  v = (ts - shift) * rh;  vv = v * v;  zz = bb + cc * vv
 *     sample = 0.0 unless zz < e2, else  z = sqrt(zz);  q = z * sM;  m = min(floor(q), M - 1);  fr = q - m
 *     sample = p[m] + (p[m + 1] - p[m]) * fr;  acc = acc + sample
 *   mval = acc / S;  where mval > 0:  mod = 1.0 - amplitude * mval;  y[i] = y[i] / mod;  model[i] = model[i] * mod
 * model starts at 1.0; a point no candidate touches comes back bit for bit.  These are the sub-samples of tls_transit_fit,
 * operation for operation, so mval at a fit's members is that fit's own, and the result equals the Python statement in
 * tests/remove_transits_spec.py bit for bit.  out_rows [n_curves][n] (may be y itself), out_model [n_curves][n] (may be NULL),
 * out_status [n_fits].  Needs no plan and leaves a prepared plan as it is.  n_fits == 0 copies the rows.  The rows are
 * processed in slabs, so device memory stays bounded for any n_curves.  TLS_E_ARG, before any device work and with the
 * outputs untouched, for a curve[f] outside [0, n_curves), a row[f] outside [0, n_k), n outside [1, 1e8], negative counts,
 * n_k outside [1, TLS_TRANSIT_FIT_MAX_ROWS], M outside [1, TLS_TRANSIT_FIT_MAX_M], n_sub outside [1, TLS_TRANSIT_FIT_MAX_SUB],
 * a k_rows that is not finite, non-decreasing and > 0, a sub or profile that is not finite, and a t that is not finite and
 * non-decreasing.  y is taken as it is. */
int tls_remove_transits(tls_ctx *ctx, const double *t, const double *y, int64_t n, int64_t n_curves, const int64_t *curve,
                        const double *period, const double *T0, const int64_t *row, const double *amplitude, const double *b,
                        const double *duration, const double *shift, int64_t n_fits, const double *k_rows,
                        const double *profile, int64_t n_k, int64_t M, const double *sub, int64_t n_sub,
                        double *out_rows /* [n_curves][n] */, double *out_model /* [n_curves][n], may be NULL */,
                        double *out_status /* [n_fits] */);

/* ---- host-only planning (no GPU needed) ------------------------------------------ */
/* Trial cells (duration x T0 positions) each period will enumerate: the data-independent
 * cost used to place shard boundaries and to report cells/s.  Mirrors core.py:50-57,143-156. */
int tls_grid_cells(const double *t, int64_t n, const double *periods, int64_t n_periods,
                   const tls_template *tmpl, const tls_params *params,
                   int64_t *cells_per_period);
/* The cost of every period for the placement of shard boundaries (tls_amd/shard.py): its trial cells (as
 * tls_grid_cells), its expected template taps -- per in-range duration: trial positions x template length x the
 * fraction of white-noise windows of scatter `sigma` whose mean depth exceeds transit_depth_min (core.py:58), the
 * cells the sliding chi^2 of core.py:59-74 is evaluated for (sigma <= 0: all of them) -- and (time_per_period, may be
 * NULL) the modelled search time of the period in shader cycles of the kernel variant tls_prepare would choose:
 * a fixed part per period (fold, sort, prefix sum: O(n) whatever the duration window) + a part per trial cell
 * (depth predicate) + a part per expected tap, coefficients measured on an MI355X.
 * The call has no dy: it plans for UNIFORM weights.  A search with per-point weights runs the classic kernel with three
 * regions (never the four-slot kernel) and leaves the LDS earlier than the kernel priced here (PERF_LOG.md, open items). */
int tls_period_costs(const double *t, int64_t n, const double *periods, int64_t n_periods,
                     const tls_template *tmpl, const tls_params *params, double sigma,
                     int64_t *cells_per_period, double *taps_per_period, double *time_per_period,
                     int64_t *workgroups_in_flight /* periods one MI355X searches side by side, may be NULL */,
                     const char *switches /* "name=value,..." of the context that will search (tls_debug_get_switches):
                                             the kernel variant and prefix-sum mode follow them; NULL: the process's */);

/* ---- multi-GPU: period grid sharded over ranks, one RCCL all-gather at the end --- */
/* rank 0 creates the 128-byte id and hands it to the other ranks by any host channel */
int tls_comm_unique_id(char id_out[128]);
int tls_comm_init(tls_ctx *ctx, int n_ranks, int rank, const char id[128]);
int tls_comm_destroy(tls_ctx *ctx);
/* What RCCL itself reports for the communicator (ncclCommCount / ncclCommUserRank / ncclCommCuDevice): an N-rank job
 * prints these, so that a run that silently used one rank cannot pass for an N-GPU run.  No communicator: 0, -1, -1. */
int tls_comm_info(tls_ctx *ctx, int *n_ranks, int *rank, int *device);
/* All-gather of the prepared search's device-resident results: every rank contributes its
 * shard (count_per_rank entries, zero padded) and receives n_ranks*count_per_rank entries of
 * chi2/row/depth in rank order.  One ncclAllGather over a packed 24 B/period buffer. */
int tls_comm_allgather_results(tls_ctx *ctx, int64_t count_per_rank, double *all_chi2,
                               int64_t *all_row, double *all_depth);
/* The same in two halves: _device enqueues pack + ncclAllGather on the context's stream and
 * returns (the gathered batch stays in HBM on every rank, the next search may be enqueued
 * right behind it); _fetch_gathered copies the most recent gather to the host and unpacks it. */
int tls_comm_allgather_device(tls_ctx *ctx, int64_t count_per_rank);
int tls_comm_fetch_gathered(tls_ctx *ctx, int64_t count_per_rank, double *all_chi2,
                            int64_t *all_row, double *all_depth);
/* Survey mode (every rank searches its own light curves): stage the latest results as slot
 * `slot` of `n_slots` with device copies on the stream -- no communication, no rank waits for
 * another -- and exchange all slots with ONE ncclAllGather at the end; _fetch_staged copies one
 * slot of that gather (n_ranks*count_per_rank entries, rank order) to the host. */
int tls_comm_stage_results(tls_ctx *ctx, int64_t count_per_rank, int64_t slot, int64_t n_slots);
int tls_comm_allgather_staged(tls_ctx *ctx, int64_t count_per_rank, int64_t n_slots);
int tls_comm_fetch_staged(tls_ctx *ctx, int64_t count_per_rank, int64_t n_slots, int64_t slot,
                          double *all_chi2, int64_t *all_row, double *all_depth);
/* small host-value collectives used by the bench harness (barrier, max over ranks) */
int tls_comm_barrier(tls_ctx *ctx);
int tls_comm_max(tls_ctx *ctx, double *value_inout);

#ifdef __cplusplus
}
#endif
#endif /* TLS_AMD_H */
