// tls_plan.hip.h -- the search planner: everything the host decides about a search before it touches the device.
//
// One value (SearchPlan) made by one function (plan_search) from the series length, the width table, the weight structure,
// the number of periods, the CU count and the switches; one pick of the kernel a launch of that plan takes (pick_kernel).
// tls_prepare reserves its buffers from the plan, enqueue launches by it, tls_plan_info reports it and tls_period_costs
// prices it: none of them restates a clause of it.  No HIP runtime call, no context and no device pointer in here: the
// file compiles into a host-only program (tests/host/plan_sweep.hip).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <numeric>
#include <thread>
#include <vector>

#include "../../include/tls_amd.h"
#include "tls_kernels.hip.h"

namespace tlsplan {

// physical constants of the duration window (reference tls_constants.py:20-25,78)
constexpr double kG = 6.673e-11;
constexpr double kRsun = 695508000.0;
constexpr double kRjup = 69911000.0;
constexpr double kMsun = 1.989 * 1e30;
constexpr double kSecondsPerDay = 86400.0;
constexpr double kFracDurationMax = 0.12;
constexpr double kPi = 3.141592653589793;

constexpr size_t kLdsPerCU = 160 * 1024;
// The four-slot kernel is taken when at least this many periods fit a CU's LDS.  Three (Tutorial 01: 100 d, 43.8 KB a period)
// already beat the classic kernel's ONE 1024-thread workgroup per CU by 18 % (1.47 against 1.79 ms, same box); in the narrow
// band where the classic kernel still fits two workgroups and this one only three, the classic one is 4 % faster (a 42-day
// probe: 0.371 against 0.386 ms) -- a series length of one day in a hundred, not special-cased.
#ifndef TLS_SLIM_MIN_SLOTS
#define TLS_SLIM_MIN_SLOTS 3
#endif
constexpr size_t kSlimMinSlots = TLS_SLIM_MIN_SLOTS;

// grid.py:9-32 with the reference's operation order (libm pow, as CPython does)
inline double t14(double R_s, double M_s, double P, bool small) {
    P = P * kSecondsPerDay;
    R_s = kRsun * R_s;
    M_s = kMsun * M_s;
    const double chord = std::pow((4 * P) / (kPi * kG * M_s), 1.0 / 3);
    const double T14max = small ? R_s * chord : (R_s + 2 * kRjup) * chord;
    double result = T14max / P;
    if (result > kFracDurationMax) result = kFracDurationMax;
    return result;
}

// The switches of a context.  Two are public (tls_options: exact_prefix, slim); the others are developer / test switches
// that select kernel variants and launch shapes for A/B runs, reached by name through tls_debug_set_switch (never part
// of the stable ABI).  -1 (band_max, prune_min_live: negative) = the library decides.
struct Switches {
    int32_t exact_prefix, slim;
    int32_t prune, screen32, no_screen, fast_slab, x_staged, split, split_batch, sort2, threads, blocks, plan_threads, t0_rot;
    int32_t reg_scan;     // four-slot kernel: stored orders stretch-major, phase 2 of a reading launch in registers (0: thread-major rows)
    int32_t dense_hoist;  // four-slot kernel, fast-mode dense depth predicate: one loop per case, band test per step, no mask for lanes without a unit (slim_dense_tile; 0: the kernel instantiations with the loop exact mode keeps)
    int32_t claim_ahead;  // four-slot kernel, the period queue's tickets (tls_slim_kernel.hip.h, slim_ticket): bit 0 a workgroup's first ticket is its index and the queue word hands out the later ones; 0: every ticket from the queue word; -1: kClaimAheadDefault
    int64_t prune_min_live;
    int64_t perm_table;  // the four-slot kernel's table of folded orders: -1 the library decides, 0 none, k > 0 at most k MiB
    double band_max;
};

// Expected fraction of trial cells that pass the depth predicate (core.py:58) on a flat, white light curve, averaged
// over the trial widths: large when the noise of a window mean, sigma/sqrt(d), is large against transit_depth_min.  It
// says how much of a period is dot products -- what the pruning variant and the fp32 screen save (pick below).
inline double passing_fraction(const std::vector<tlsdev::WidthEntry>& widths, double sigma, double depth_min) {
    if (!(sigma > 0) || widths.empty()) return 0.0;
    double acc = 0.0;
    for (const auto& we : widths) acc += 0.5 * std::erfc(depth_min * std::sqrt((double)we.width) / sigma / std::sqrt(2.0));
    return acc / (double)widths.size();
}
// fp32 screen of the dot products (tlsdev::screen_cells) admissible: LDS-resident series, uniform weights, every sample
// e = 1 - flux the exact sum of two fp32 halves (flux in [0.5, 2] and |e| < 2^-5)
inline bool screen_admissible(bool resident, bool uniform, double e_abs_max) {
    return resident && uniform && e_abs_max < 0.03125;
}
// Which variant of the LDS-resident search kernel a launch takes, from the expected passing fraction f of the depth
// predicate.  Round 4, 90-day configuration, same box, ms (plain / fp32 screen / pruning): 50 ppm (f = 0.09) 1.19 / 1.23 /
// 1.61; 75 ppm (0.16) 1.67 / 1.62 / 1.87; 100 ppm (0.20) 2.10 / 1.94 / 2.14; 150 ppm (0.28) 2.62 / 2.34 / 2.37; 200 ppm
// (0.32) 2.94 / 2.54 / 2.47; 300 ppm (0.38) 3.22 / 2.76 / 2.58; 500 ppm (0.42) 3.61 / 2.93 / 2.75.  The
// screen halves the FMA instructions of the dot products but adds a split pass and a valuation pass per period (DESIGN
// section 4): it pays where the dot products dominate and the pruning passes do not pay yet.
// switch prune = 0/1 and ::screen32 = 0/1 force either choice (tests run all three variants).
constexpr double kScreenFromFraction = 0.13, kPruneFromFraction = 0.24, kPruneFromFractionBesideScreen = 0.30;
inline bool pruning_pays(const Switches& opt, const std::vector<tlsdev::WidthEntry>& widths, double sigma, double depth_min, bool resident,
                  bool screen_ok = false) {
    if (!resident) return false;   // (the bound's look-ups in X want the series in LDS: no slab instantiation)
    if (opt.prune >= 0) return opt.prune != 0;
    if (!(sigma > 0) || widths.empty()) return false;
    for (const auto& we : widths) if (!we.prunable) return false;
    if (opt.screen32 >= 0) screen_ok = screen_ok && opt.screen32 != 0;
    return passing_fraction(widths, sigma, depth_min) >= (screen_ok ? kPruneFromFractionBesideScreen : kPruneFromFraction);
}
inline bool screen_pays(const Switches& opt, const std::vector<tlsdev::WidthEntry>& widths, double sigma, double depth_min, bool admissible) {
    if (!admissible) return false;
    if (opt.screen32 >= 0) return opt.screen32 != 0;
    return passing_fraction(widths, sigma, depth_min) >= kScreenFromFraction;
}

// Fast prefix-sum mode: half-width of the band around transit_depth_min inside which the plain scan
// cannot decide a window -- 1.25 x the bound 2^-53 c_max on |dX/d - mean_reference| (c_max = (n + W) max|flux| bounds the
// reference's running sum), plus 1e-14 for what the bound leaves out (the plain scan's own rounding, <= ~20 * 2^-53 *
// max|X| / d, and the reference's division; rounds 3 and early 4 shipped 2 x: twice the second attempts for no safety).
// (round 4, when a band hit cost a second search of the period -- Kepler full grid, same box: 0.35 -> 244 ms, 0.1 -> 241,
// 0.01 -> 240, never -> 249.  Round 5: a hit costs one exact prefix pass (band_window in tls_kernels.hip.h) -- every 16th
// Kepler period: 0 (all exact) 16.97 ms, 0.1 14.22, 1 14.02, 10 14.04, never 14.02; TESS 3.01 / 2.72 / 2.72 / 2.72 / 2.73.)
constexpr double kBandMax = 1.0;
constexpr double kBandHitCost = 0.15;   // of a period: the exact prefix pass and the few windows it decides
inline double fast_mode_eps(int64_t M, double y_abs_max) {
    return 1.25 * (1.1102230246251565e-16 * ((double)M * y_abs_max)) + 1e-14;
}
// Expected number of windows of width row k inside that band, as a prefix over the width table: n_pos * 2 eps * density of
// the window mean at depth_min (a flat, white light curve: mean of 1 - flux ~ N(0, sigma^2 / d)).  A period's expectation
// is pre[k_hi] - pre[k_lo]; above band_max the period starts in exact mode (kernel), and it weighs on the queue order (host).
// n_pos of a row is (M - width) / xth + 1, the same for every period of the plan.
inline void band_prefix_for(const std::vector<tlsdev::WidthEntry>& widths, double sigma, double depth_min, double eps,
                     std::vector<double>& pre, int64_t M = -1) {
    pre.assign(widths.size() + 1, 0.0);
    for (size_t k = 0; k < widths.size(); ++k) {
        const auto& we = widths[k];
        const double n_pos = M >= 0 ? (double)((M - we.width) / we.xth + 1) : (double)we.n_pos;
        const double sd = sigma / std::sqrt((double)we.width), z = depth_min / sd;
        pre[k + 1] = pre[k] + n_pos * 2.0 * eps * std::exp(-0.5 * z * z) / (sd * 2.5066282746310002);
    }
}

// In-range width window of every period (core.py:143-156) and its trial-cell count.
// The same for every period of a grid (what tls_prepare and tls_grid_cells need): the in-range rows [k_lo, k_hi)
// of the ascending width table by binary search, the dense rows [k_lo, k_x), and the trial-cell count from a
// prefix sum over the table -- per period two pow() calls (t14, kept in the reference's operation order) and a few
// dozen instructions instead of a walk over all widths.  Long grids are cut into slices for a few host threads
// (a Kepler-size grid of 182 388 periods: 21 ms on one core).  Returns false on a non-positive or non-finite period.
struct GridPlan {
    int64_t cells = 0, pairs = 0;
};
inline bool plan_periods(const std::vector<tlsdev::WidthEntry>& widths, const tls_params* params, const double* periods,
                  int64_t n_periods, double length, int64_t n, int64_t M, tlsdev::PeriodRows* prow, int64_t* cost,
                  GridPlan* total, int plan_threads = -1) {
    const int nw = (int)widths.size();
    std::vector<int> wd((size_t)nw);
    std::vector<int64_t> prefix((size_t)nw + 1, 0);
    int first_strided = nw;   // xth = int(width * margin) never decreases with the width (core.py:50-55)
    for (int k = 0; k < nw; ++k) {
        wd[(size_t)k] = widths[(size_t)k].width;
        prefix[(size_t)k + 1] = prefix[(size_t)k] + ((M - widths[(size_t)k].width) / widths[(size_t)k].xth + 1);
        if (widths[(size_t)k].xth != 1 && first_strided == nw) first_strided = k;
    }
    for (int k = first_strided; k < nw; ++k)
        if (widths[(size_t)k].xth == 1) first_strided = -1;   // not monotone (cannot happen): per-row walk below
    auto slice = [&](int64_t p0, int64_t p1, GridPlan* out, bool* ok) {
        GridPlan g;
        for (int64_t p = p0; p < p1; ++p) {
            const double P = periods[p];
            if (!(P > 0) || !std::isfinite(P)) { *ok = false; return; }
            const double duration_max = t14(params->R_star_max, params->M_star_max, P, false);
            const double duration_min = t14(params->R_star_min, params->M_star_min, P, true);
            const double naive = length / P;
            const double correction = (naive + 1) / naive;
            const double lo = std::floor(duration_min * (double)n);
            const double hi = std::ceil(duration_max * (double)n * correction);
            const int dlo = (int)std::max(-2.0e9, std::min(2.0e9, lo));
            const int dhi = (int)std::max(-2.0e9, std::min(2.0e9, hi));
            const int k_lo = (int)(std::lower_bound(wd.begin(), wd.end(), dlo) - wd.begin());
            const int k_hi = std::max(k_lo, (int)(std::upper_bound(wd.begin(), wd.end(), dhi) - wd.begin()));
            int k_x = std::min(k_hi, std::max(k_lo, first_strided));
            if (first_strided < 0) {
                k_x = k_lo;
                for (int k = k_lo; k < k_hi; ++k) if (widths[(size_t)k].xth == 1) k_x = k + 1;
            }
            const int64_t c = prefix[(size_t)k_hi] - prefix[(size_t)k_lo];
            if (prow) { prow[p].k_lo = k_lo; prow[p].k_hi = k_hi; prow[p].k_x = k_x; prow[p].pad = 0; }
            if (cost) cost[p] = c;
            g.cells += c; g.pairs += k_hi - k_lo;
        }
        *out = g;
    };
    unsigned n_threads = 1;
    if (n_periods >= 4096) {
        n_threads = std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 8u);
        n_threads = (unsigned)std::min<int64_t>(n_threads, n_periods / 2048);
        if (plan_threads > 0) n_threads = (unsigned)std::max(1, std::min(64, plan_threads));
    }
    std::vector<GridPlan> part(n_threads);
    std::vector<char> ok(n_threads, 1);
    if (n_threads <= 1) {
        bool good = true;
        slice(0, n_periods, &part[0], &good);
        ok[0] = good;
    } else {
        std::vector<std::thread> pool;
        std::vector<bool*> flags;
        std::unique_ptr<bool[]> good(new bool[n_threads]);
        for (unsigned i = 0; i < n_threads; ++i) {
            good[i] = true;
            const int64_t p0 = n_periods * i / n_threads, p1 = n_periods * (i + 1) / n_threads;
            pool.emplace_back(slice, p0, p1, &part[i], &good[i]);
        }
        for (auto& th : pool) th.join();
        for (unsigned i = 0; i < n_threads; ++i) ok[i] = good[i];
    }
    for (unsigned i = 0; i < n_threads; ++i) {
        if (!ok[i]) return false;
        total->cells += part[i].cells; total->pairs += part[i].pairs;
    }
    return true;
}

// the widest trial width made even: the pad W behind the series (core.py:114-116); the folded series is M = n + W long
inline int64_t padded_width(const std::vector<tlsdev::WidthEntry>& widths) {
    const int64_t W = widths.back().width;
    return W + W % 2;
}
// LDS header of the classic and the slab kernels: fixed part + per-row live counters and batch prefix (+ the batch counter)
inline size_t lds_header_bytes(size_t n_widths) {
    return ((size_t)tlsdev::kFixedHeader + 4 * (3 * n_widths + 2) + 15) / 16 * 16;
}
// sort buckets of the general fold_and_sort for a series of n points (the resident kernel uses n; the slab variant
// what its LDS holds)
inline int64_t sort_buckets_for(int64_t n, size_t n_widths) {
    return std::min<int64_t>(n, (int64_t)((kLdsPerCU - lds_header_bytes(n_widths)) / 4));
}
// smallest and largest time stamp
inline void time_range(const double* t, int64_t n, double& t_min, double& t_max) {
    t_min = t_max = t[0];
    for (int64_t i = 1; i < n; ++i) { t_min = std::min(t_min, t[i]); t_max = std::max(t_max, t[i]); }
}

// the four-slot kernel's ticket protocol where the switch claim_ahead leaves it to the library (PERF_LOG.md: the one part kept)
constexpr int kClaimAheadDefault = 1;
inline int claim_ahead_bits(const Switches& opt) { return opt.claim_ahead < 0 ? kClaimAheadDefault : (opt.claim_ahead & 1); }

// the table of folded orders of a four-slot plan is held up to this size (switch perm_table: another cap, or none)
constexpr size_t kPermTableMaxBytes = (size_t)1 << 30;

// work order of the period queue: most expensive first (longest-processing-time first), ties in grid order --
// a stable LSD radix sort of the 32-bit key (max cost - cost), three passes of 11 bits
inline void order_by_cost(const std::vector<int64_t>& cost, std::vector<int>& order) {
    const size_t np = cost.size();
    order.resize(np);
    int64_t cmax = 0;
    for (size_t p = 0; p < np; ++p) cmax = std::max(cmax, cost[p]);
    if (cmax >= (1LL << 33)) {   // (absurdly long series: comparison sort)
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cost[(size_t)a] > cost[(size_t)b]; });
        return;
    }
    std::vector<unsigned long long> key(np), tmp(np);
    for (size_t p = 0; p < np; ++p) key[p] = ((unsigned long long)(cmax - cost[p]) << 31) | (unsigned long long)p;   // p < 2^31
    for (int pass = 0; pass < 3; ++pass) {
        const int shift = 31 + 11 * pass;
        if (pass > 0 && (cmax >> (11 * pass)) == 0) break;
        size_t hist[2049] = {0};
        for (size_t p = 0; p < np; ++p) ++hist[((key[p] >> shift) & 2047u) + 1];
        for (int b = 0; b < 2048; ++b) hist[b + 1] += hist[b];
        for (size_t p = 0; p < np; ++p) tmp[hist[(key[p] >> shift) & 2047u]++] = key[p];
        key.swap(tmp);
    }
    for (size_t p = 0; p < np; ++p) order[p] = (int)(key[p] & 0x7fffffffull);
}

// Work order: most expensive first.  A period commensurate with the cadence of a regularly sampled series piles
// the phases onto a few values and its sort costs several ordinary periods: such a period
// goes to the head of the queue, where its long run overlaps everything else instead of ending the launch.
inline void order_queue(const double* t, int64_t n, const double* periods, int64_t n_periods, const std::vector<tlsdev::WidthEntry>& widths,
                        const tlsdev::PeriodRows* prow, const std::vector<int64_t>& cost, bool uniform, int64_t M, double flux_sigma,
                        double y_abs_max, double depth_min, const Switches& opt, std::vector<int>& order) {
    std::vector<int64_t> queue_cost(cost);
    bool regular = n >= 64;
    double dt = 0.0;
    if (regular) {
        dt = (t[n - 1] - t[0]) / (double)(n - 1);
        regular = dt > 0;
        for (int64_t i = 1; i < n && regular; ++i) regular = std::fabs((t[i] - t[i - 1]) - dt) <= 1e-3 * dt;
    }
    if (regular) {
        // (the four-slot kernel ranks piles from 9 points on by themselves, 2-3 x an ordinary period: a short series
        // looks for smaller piles and higher resonances -- flagging too many only reorders the queue)
        const bool fine_piles = uniform && n <= (int64_t)tlsdev::kSlimThreadsWide * tlsdev::kSlimPer;
        const int k_max = fine_piles ? 8 : 4;
        const double a_max = (double)n / (fine_piles ? 9.0 : 48.0);       // `a` distinct phase values: piles of n / a points
        const double n_buckets = fine_piles ? 0.5 * (double)n : (double)sort_buckets_for(n, widths.size());
        const double drift = (fine_piles ? 8.0 : 4.0) / ((double)n * n_buckets);   // a pile's phase range, in buckets, over the series
        const double inv_dt = 1.0 / dt;
        for (int64_t p = 0; p < n_periods; ++p) {
            const double r = periods[p] * inv_dt;             // samples per period
            for (int k = 1; k <= k_max; ++k) {
                const double rk = r * k, a = std::floor(rk + 0.5);   // r ~ a / k
                if (a > a_max) break;
                if (a < 1) continue;
                // n |k/a - 1/r| n_buckets < limit  <=>  |r k - a| < limit a r / (n n_buckets)
                if (std::fabs(rk - a) < drift * a * r) { queue_cost[(size_t)p] += 50 * cost[(size_t)p]; break; }
            }
        }
    }
    // Fast prefix-sum mode: a period whose windows are likely to meet the undecided band pays a second attempt
    // pass (kBandHitCost of itself); among periods of similar cost the likelier ones start first, so that the extra
    // passes fall into the body of the launch and not into its last round.  (Only the order: which mode a period takes
    // never depends on it.)  The expectation is band_prefix_for's, as in enqueue; the LDS-resident kernel has no
    // per-period expectation (every period starts in fast mode): the same weight orders its queue.
    if (flux_sigma > 0 && opt.exact_prefix != 1) {
        std::vector<double> pre;
        band_prefix_for(widths, flux_sigma, depth_min, fast_mode_eps(M, y_abs_max), pre, M);
        const double band_max = opt.band_max >= 0 ? opt.band_max : kBandMax;
        for (int64_t p = 0; p < n_periods; ++p) {
            const double lambda = pre[(size_t)prow[(size_t)p].k_hi] - pre[(size_t)prow[(size_t)p].k_lo];
            if (lambda > band_max) continue;                                   // (starts in exact mode: no second attempt)
            queue_cost[(size_t)p] += (int64_t)(kBandHitCost * std::min(1.0, lambda) * (double)cost[(size_t)p]);
        }
    }
    order_by_cost(queue_cost, order);
}

// Everything the host decides about a search from the series length, the width table, the weight structure, the number of
// periods, the CU count and the switches (plan_search below).  tls_ctx holds one; so does nobody else for long.
struct SearchPlan {
    // sizes
    int n = 0, W = 0, M = 0, n_periods = 0, n_widths = 0;
    bool uniform = true;
    bool short_rows = false;          // a template row shorter than its width (tlsdev::short_row_tail): the plain classic or slab kernel only
    // classic launch (LDS-resident or slab)
    int region_pad = 0, hdr_bytes = 0;
    bool resident = true;
    int nb = 0;
    size_t lds_bytes = 0;
    int threads = 512, blocks = 0;
    int per_cu = 1;                   // workgroups whose LDS fits a CU side by side (resident; a slab plan: one)
    // four-slot kernel (tls_slim_kernel.hip.h)
    int slim_blocks = 0;              // > 0: the plan fits it: its workgroups in flight
    size_t slim_lds = 0;              // ... its dynamic LDS
    int slim_threads = 256;           // ... its workgroup size: 256 (four or three to a CU) or 512 (two to a CU: series of 5-10 k points)
    int slim_slots = 0;               // ... and how many of them a CU holds
    int slim_perm_per = 0;            // the layout of the plan's stored orders (SearchArgs::perm_per): > 0 stretch-major
    size_t perm_table_want = 0;       // entries of the table of folded orders the plan wants; 0: none
    // slab: the series in HBM, staged through LDS tile by tile
    int tile_len = 0, tile_halo = 0;
    bool sort2 = false;               // two-level sort
    int cumsum_round = 2 * tlsdev::kCumsumChunk;
    size_t scratch_doubles = 0;       // the workgroups' (a two-role plan: the batch's) slabs
    bool any_oversize = false;        // a row wider than half a tile: evaluated straight from the slab
    // two-role slab path: fold role + search role per batch of periods
    bool split = false;               // the plan supports it (single-curve launches take it)
    bool split_fast = false;          // the two roles may run fast prefix-sum mode (uniform weights, X at staging, dot products on X)
    int split_blocks = 0;             // workgroups of its launches (not capped by the number of periods: tiles are items too)
    int split_batch = 0;              // periods per batch: as many slabs are held in HBM
    int64_t split_max_items = 0;      // most (period, tile, row part) items of any batch
    std::vector<unsigned int> tile_prefix;   // [n_periods + 1] tiles in front of work item w (queue order)
    // the rest
    size_t list_stride = 0;
    int p2_shift = 4;
    long long prune_min_live = 256;   // live units per period (tile) from which pruning pays; switch prune_min_live overrides
};

// The plan of a search.  Marks the `oversize` rows of `widths` and fills their per-width work units; with `prow` (the
// periods' rows, plan_periods) and `order` (the queue, order_queue) also every period's own tile length (PeriodRows::pad)
// and the tile prefix of a two-role plan -- a caller that only wants the shape (tls_period_costs) passes neither.
// Returns nullptr, or why the series cannot be searched (`plan` then holds its sizes and `resident`, nothing else).
inline const char* plan_search(SearchPlan& plan, int64_t n, std::vector<tlsdev::WidthEntry>& widths, bool uniform, int64_t n_periods,
                               int n_cu, const Switches& opt, tlsdev::PeriodRows* prow = nullptr, const int* order = nullptr) {
    plan = SearchPlan();
    const int64_t W = padded_width(widths), M = n + W;
    plan.n = (int)n; plan.W = (int)W; plan.M = (int)M; plan.n_periods = (int)n_periods;
    plan.n_widths = (int)widths.size(); plan.uniform = uniform;
    for (const auto& we : widths) plan.short_rows = plan.short_rows || we.q_len < we.width;
    const size_t regions = uniform ? 2 : 3;
    int widest_stride = 1;  // of the tiled rows: sizes the pads behind the folded series and the tile halo
    for (const auto& we : widths) if (we.tiled) widest_stride = std::max(widest_stride, we.xth);
    plan.region_pad = tlsdev::region_pad_for(widest_stride);
    const size_t region_doubles = (size_t)(M + 1 + plan.region_pad);
    const size_t hdr = lds_header_bytes(widths.size());
    const size_t resident_bytes = hdr + regions * 8 * region_doubles;
    plan.hdr_bytes = (int)hdr;
    plan.resident = resident_bytes <= kLdsPerCU && n <= 65535;
    if (plan.resident) {
        plan.nb = (int)n;
        plan.lds_bytes = resident_bytes;
        const size_t per_cu = kLdsPerCU / resident_bytes;
        plan.per_cu = (int)per_cu;
        plan.threads = per_cu >= 2 ? 512 : 1024;
        if (opt.threads > 0) plan.threads = std::max(64, std::min(1024, opt.threads / 64 * 64));   // developer switch
        const size_t wg_per_cu = std::min<size_t>(per_cu, 2048 / (size_t)plan.threads);
        plan.blocks = (int)std::min<int64_t>(std::max<int64_t>(n_periods, 1), (int64_t)wg_per_cu * n_cu);
        if (opt.blocks > 0) plan.blocks = std::max(1, std::min(plan.blocks, opt.blocks));   // developer switch
        // Four (at least three) 256-thread workgroups per CU, phase 3 on X alone (tls_slim_kernel.hip.h): uniform weights, and
        // the period's one region + header within a quarter (a third) of the LDS.  (switch slim = 0: never.)
        // (auto: only while the library also decides between the classic kernel's variants -- an explicit switch prune
        // or ::screen32 selects among THOSE; slim = 1 forces this kernel wherever neither pruning nor the screen is taken)
        // (exact prefix-sum mode throughout is the classic kernel's: this one values its cells on the plain scan, and keeps
        // the exact prefix sum for the windows the plain scan cannot decide)
        const bool slim_wanted = opt.exact_prefix != 1 && (opt.slim == 1 || (opt.slim < 0 && opt.prune < 0 && opt.screen32 < 0));
        // (a table with a short row: the classic kernel, whose dot-product phase forms the row's tail term)
        if (uniform && slim_wanted && opt.threads <= 0 && !plan.short_rows) {
            const long long need = tlsdev::slim_lds_bytes((int)n, (int)M, plan.region_pad, (int)widths.size());
            // (a series beyond 5120 points -- 107-200 d at 30 min, two TESS sectors at 10 min --: the same kernel with 512-thread
            // workgroups, two to a CU, where the classic kernel runs ONE 1024-thread workgroup per CU; round 6)
            const long long need_wide = tlsdev::slim_lds_bytes((int)n, (int)M, plan.region_pad, (int)widths.size(), tlsdev::kSlimThreadsWide);
            if (need > 0 && kSlimMinSlots * (size_t)need <= kLdsPerCU) {
                plan.slim_lds = (size_t)need; plan.slim_threads = tlsdev::kSlimThreads;
                plan.slim_slots = (int)std::min<size_t>(4, kLdsPerCU / (size_t)need);
                plan.slim_blocks = (int)std::min<int64_t>(std::max<int64_t>(n_periods, 1), (int64_t)plan.slim_slots * n_cu);
                if (opt.blocks > 0) plan.slim_blocks = std::max(1, std::min(plan.slim_blocks, opt.blocks));
            } else if (need == 0 && need_wide > 0 && 2 * (size_t)need_wide <= kLdsPerCU) {
                plan.slim_lds = (size_t)need_wide; plan.slim_threads = tlsdev::kSlimThreadsWide;
                plan.slim_slots = 2;
                plan.slim_blocks = (int)std::min<int64_t>(std::max<int64_t>(n_periods, 1), (int64_t)plan.slim_slots * n_cu);
                if (opt.blocks > 0) plan.slim_blocks = std::max(1, std::min(plan.slim_blocks, opt.blocks));
            }
        }
    } else {
        // the folded series lives in a per-workgroup HBM slab; phase 3 stages it through LDS in
        // tiles of `tile_len` window-start positions plus a halo of the widest window
        // sort histogram: one bucket per point while the counters fit the LDS (fewer points per
        // bucket = fewer comparisons in the in-bucket ranking)
        // (as fine as the LDS allows: a NEARLY commensurate period spreads its piles over neighbouring buckets, and fine
        // buckets keep them below the size from which the counting rank is left; what LDS remains behind the counters
        // stages piled-up buckets for the workgroup sort, fold_and_sort)
        // One 1024-thread workgroup per CU with all of its LDS (two 512-thread ones with half each were measured in rounds 3
        // and 4 and lost: more tiles, more halo staged; the switch is gone).
        const size_t lds_budget = kLdsPerCU;
        plan.nb = (int)std::min<int64_t>(n, (int64_t)((lds_budget - hdr) / 4));
        size_t halo = (size_t)W + (size_t)(tlsdev::kR - 1) * (size_t)std::max(widest_stride, tlsdev::kMaxTiledStride) + 2 * tlsdev::kU + 4;
        const size_t unit = (size_t)tlsdev::kR * tlsdev::kWave;  // tile bounds: multiples of 320
        {
            // Very long series (N beyond ~150 k with the default duration grid): the widest windows are longer
            // than an LDS tile.  Rows wider than half the tile capacity are marked `oversize`: their (few,
            // widely strided) trial positions are listed and evaluated straight from the slab, one window per
            // wavefront, and the tile halo only has to cover the other rows.  The reference has no size
            // limit (core.py:96-188).
            const size_t cap1 = (lds_budget - hdr) / 8 / ((uniform ? 1 : 2));
            if (cap1 < halo + 4 * unit) {
                const size_t halo_cap = cap1 / 2;
                size_t widest_fit = 1;
                int stride_fit = 1;
                for (auto& we : widths) {
                    const size_t need = (size_t)we.width + (size_t)(tlsdev::kR - 1) * (size_t)std::max(we.tiled ? we.xth : 1, tlsdev::kMaxTiledStride) + 2 * tlsdev::kU + 4;
                    if (need > halo_cap) { we.oversize = 1; we.tiled = 0; we.prunable = 0; }
                    else { widest_fit = std::max(widest_fit, (size_t)we.width); if (we.tiled) stride_fit = std::max(stride_fit, we.xth); }
                }
                widest_stride = stride_fit;
                plan.region_pad = tlsdev::region_pad_for(widest_stride);
                halo = widest_fit + (widest_fit & 1) + (size_t)(tlsdev::kR - 1) * (size_t)std::max(widest_stride, tlsdev::kMaxTiledStride) + 2 * tlsdev::kU + 4;
            }
        }
        // staged per tile: e (or e*w), and w for per-point weights.  The prefix sum takes the samples' place for the
        // predicate pass (or is formed in place from the staged flux: fast mode), the samples follow for the dot products --
        // two stagings per tile, but fewer and larger tiles than with X staged beside the samples (TESS: 2 instead of 3,
        // -8 %; Kepler-size: 7 instead of 82, most of a tile is halo; that variant was dropped in round 6).
        const size_t buffers = uniform ? 1 : 2;
        if ((lds_budget - hdr) / 8 / buffers < halo + unit) return "widest transit window does not fit the LDS tile";
        const size_t cap_doubles = (lds_budget - hdr) / 8 / buffers;
        const size_t cap_tile = (cap_doubles - halo) / unit * unit;
        const size_t n_tiles = ((size_t)M + cap_tile - 1) / cap_tile;
        size_t tile = (((size_t)M + n_tiles - 1) / n_tiles + unit - 1) / unit * unit;
        if (tile > cap_tile) tile = cap_tile;
        plan.tile_len = (int)tile; plan.tile_halo = (int)halo;
        // Per period the halo only has to cover the widest IN-RANGE window (core.py:148-156): long periods try
        // narrow windows only, so their tiles can be longer (fewer tiles, less of the slab staged twice).  The
        // LDS tile stays `tile + halo` doubles; PeriodRows::pad carries the period's own tile length.
        {
            const size_t staged = tile + halo;
            // (widths ascend and strides never decrease with them: the widest in-range window and the largest stride
            // of a period are those of its last in-range row that is not oversize -- one table over k_hi, one look-up
            // per period instead of a walk over its rows)
            const size_t nw = widths.size();
            std::vector<int> tile_for_khi(nw + 1, 0);
            {
                size_t wmax = 1; int stride_p = 1;
                for (size_t k = 0; k < nw; ++k) {
                    const auto& we = widths[k];
                    if (!we.oversize) {
                        wmax = std::max(wmax, (size_t)we.width);
                        if (we.tiled) stride_p = std::max(stride_p, we.xth);
                    }
                    const size_t halo_p = wmax + (wmax & 1) + (size_t)(tlsdev::kR - 1) * (size_t)std::max(stride_p, tlsdev::kMaxTiledStride) + 2 * tlsdev::kU + 4;
                    if (halo_p >= halo) continue;   // (0: the plan's tile length)
                    const size_t cap_p = (staged - halo_p) / unit * unit;
                    const size_t tiles_p = ((size_t)M + cap_p - 1) / cap_p;
                    size_t tile_p = (((size_t)M + tiles_p - 1) / tiles_p + unit - 1) / unit * unit;
                    if (tile_p > cap_p) tile_p = cap_p;
                    if (tile_p > tile) tile_for_khi[k + 1] = (int)tile_p;
                }
            }
            for (int64_t p = 0; prow && p < n_periods; ++p) {
                tlsdev::PeriodRows& pr = prow[(size_t)p];
                // (the running maxima above start at row 0, the period's at k_lo: the same whenever the period has a row)
                pr.pad = pr.k_hi > pr.k_lo ? tile_for_khi[(size_t)pr.k_hi] : 0;
            }
        }
        const size_t cumsum_bytes = 8 * ((size_t)plan.cumsum_round + 4);
        plan.lds_bytes = hdr + std::max<size_t>(std::max<size_t>(4 * (size_t)plan.nb, cumsum_bytes),
                                                buffers * 8 * (tile + halo));
        plan.threads = 1024;
        if (opt.threads > 0) plan.threads = std::max(64, std::min(1024, opt.threads / 64 * 64));   // developer switch
        plan.blocks = (int)std::min<int64_t>(std::max<int64_t>(n_periods, 1), (int64_t)n_cu);
        if (opt.blocks > 0)   // developer switch: workgroups in flight (memory-system experiments)
            plan.blocks = std::max(1, std::min(plan.blocks, opt.blocks));
        // two-level sort with sequential HBM accesses (fold_and_sort_tiled) when its LDS windows fit
        const size_t sort2_bytes = hdr + (size_t)tlsdev::sort2_lds_bytes((int)n, plan.threads);
        plan.sort2 = sort2_bytes <= lds_budget && opt.sort2 != 0;
        if (plan.sort2) plan.lds_bytes = std::max(plan.lds_bytes, sort2_bytes);
        // Two-role slab kernel: every workgroup folds periods into per-period slabs, then searches
        // (period, tile) items; the periods go through it in batches that hold one slab per period in HBM (as many periods as
        // fit `kSplitSlabBytes`, at least four rounds of workgroups; all of them when the grid is small).
        // WHEN it is used (measured on one MI355X, same box, against the one-workgroup-per-period kernel): it wins where a
        // GPU holds few periods of a long series -- the shard of a multi-GPU job -- because a period is then searched by
        // several workgroups (260 periods of N = 70 128: 0.61 vs 0.79 ms); on a full grid the one-kernel path keeps every
        // CU in a different phase and needs no hand-off (TESS 2.99 vs 3.50 ms, Kepler sample 5.37 vs 5.43 ms; 713 periods of
        // N = 70 128, 2.8 rounds: 1.37 vs 1.63 ms; 308 periods of the TESS-size series: 0.53 ms both ways).  Hence: up to one
        // and a half rounds of periods -> two-role kernel.  TLS_SPLIT=0/1 forces the choice (A/B, tests).
        plan.split_blocks = n_cu;
        if (opt.blocks > 0) plan.split_blocks = std::max(1, std::min(plan.split_blocks, opt.blocks));
        {
            // WHICH launches take it.  The mode of a period never depends on the launch shape (enqueue), so the two roles must
            // be able to run a period in the mode the one-workgroup kernel gives it: fast mode with X formed at tile-staging
            // time and the dot products on X (`split_fast`: uniform weights, no row wider than an LDS tile, an even number of
            // points), or a plan that is exact throughout.  Where that holds, a SHORT launch whose last round of periods would
            // be partly filled -- the share of a rank of a multi-GPU search, a few hundred periods of a long series -- goes
            // through the two roles: 3.6 items per workgroup instead of 1.2 periods, and the launch ends within a tile's work
            // instead of a whole period's.  Measured (round 6, TESS-size series, same box, one-workgroup kernel / two roles):
            // 307 periods 0.583 / 0.479 ms, 411 periods 0.522 / 0.489; but 256 periods (one full round) 0.567 / 0.623 and 512
            // 0.484 / 0.509 -- a launch of whole rounds has no partly filled round to repair and pays the hand-off (slabs read
            // across XCDs, the ready flags) for nothing; a full grid stays with the one-workgroup kernel (every CU in a
            // different phase).  Hence: up to four rounds, and the last one filled to between 1 and 70 %.
            // switch split = 0 / 1 forces the choice (A/B, tests).
            for (const auto& we : widths) plan.any_oversize = plan.any_oversize || we.oversize != 0;
            const bool all_exact = opt.exact_prefix == 1 || opt.fast_slab == 0;
            plan.split_fast = uniform && !plan.any_oversize && (n & 1) == 0 && !all_exact && opt.x_staged != 0;
            const int64_t last_round = n_periods % (int64_t)plan.split_blocks;
            const bool short_launch = n_periods <= 4 * (int64_t)plan.split_blocks && last_round > 0 && 10 * last_round <= 7 * (int64_t)plan.split_blocks;
            plan.split = n_periods > 0 && (opt.split >= 0 ? opt.split != 0 : (all_exact || plan.split_fast) && short_launch);
            const size_t slab_bytes = regions * ((region_doubles + 1) & ~(size_t)1) * 8;
            constexpr size_t kSplitSlabBytes = (size_t)12 << 30;
            int64_t batch = std::max<int64_t>((int64_t)(kSplitSlabBytes / slab_bytes), (int64_t)4 * plan.split_blocks);
            if (opt.split_batch > 0) batch = opt.split_batch;
            plan.split_batch = (int)std::min<int64_t>(std::max<int64_t>(n_periods, 1), batch);
            if (plan.split && prow && order) {
                plan.tile_prefix.assign((size_t)n_periods + 1, 0u);
                for (int64_t wk = 0; wk < n_periods; ++wk) {
                    const tlsdev::PeriodRows& pr = prow[(size_t)order[(size_t)wk]];
                    const size_t tl = pr.pad > 0 ? (size_t)pr.pad : tile;      // the kernel's tile length of this period
                    plan.tile_prefix[(size_t)wk + 1] = plan.tile_prefix[(size_t)wk] + (unsigned int)(((size_t)M + tl - 1) / tl);
                }
                for (int64_t lo = 0; lo < n_periods; lo += plan.split_batch) {
                    const int64_t hi = std::min<int64_t>(n_periods, lo + plan.split_batch);
                    plan.split_max_items = std::max<int64_t>(plan.split_max_items, (int64_t)plan.tile_prefix[(size_t)hi] - (int64_t)plan.tile_prefix[(size_t)lo]);
                }
            }
        }
        const size_t scratch_blocks = std::max<size_t>((size_t)plan.blocks, plan.split ? (size_t)plan.split_batch : 0);
        plan.scratch_doubles = scratch_blocks * regions * (region_doubles + 1) + 16;
    }
    // per-width work units of phase 3 (M is fixed for the plan, so these are period independent)
    // and the layout of one workgroup's live-unit lists: every unit of every width has a slot
    size_t list_cap = 0;
    for (auto& we : widths) {
        const int64_t n_pos = (M - we.width) / we.xth + 1;
        const int64_t r = we.tiled ? tlsdev::kR : 1;
        we.n_pos = (int)n_pos;
        we.n_chunks = (int)((n_pos + r - 1) / r);
        we.list_base = (int)list_cap;
        we.inv_d = 1.0 / (double)we.width;
        list_cap += (size_t)we.n_chunks;
    }
    plan.list_stride = (list_cap + 63) / 64 * 64;
    {
        // the table of folded orders of a four-slot plan, within its budget; a plan without one sorts in every launch
        size_t want = 0;
        if (plan.slim_blocks > 0 && opt.perm_table != 0) {
            const size_t entries = (size_t)n_periods * (size_t)tlsdev::slim_perm_row(plan.slim_threads);
            const size_t cap = opt.perm_table > 0 ? (size_t)opt.perm_table << 20 : kPermTableMaxBytes;
            if (entries * sizeof(unsigned short) <= cap) want = entries;
        }
        plan.perm_table_want = want;
        // the layout of the plan's stored orders (table rows, a survey group's stash): stretch-major where the fast-mode
        // scan's stretch fits a thread's entries (tls_slim_kernel.hip.h), thread-major otherwise (and by switch reg_scan = 0)
        const int per = plan.slim_blocks > 0 ? tlsdev::slim_scan_per(plan.slim_threads, (int)M) : 0;
        plan.slim_perm_per = (opt.reg_scan != 0 && per <= tlsdev::kSlimPer && W <= n) ? per : 0;
    }
    plan.prune_min_live = opt.prune_min_live >= 0 ? (long long)opt.prune_min_live : 256;
    plan.p2_shift = 4;  // block length of the coarse prefix sum of e^2: at most kP2MaxBlocks blocks
    while ((((size_t)M + ((size_t)1 << plan.p2_shift) - 1) >> plan.p2_shift) > (size_t)tlsdev::kP2MaxBlocks) ++plan.p2_shift;
    return nullptr;
}

// The variants of the classic resident kernel the flux of the next launch asks for, from its scatter (a batch: the mean
// over the curves of its group).  `screen_admits`: what screen_admissible says of that flux, evaluated once, here.
// `prune_beside_screen`: pruning competes with an admissible screen (threshold 0.30) and not with the plain kernel (0.24).
struct FluxChoice {
    double sigma = 0.0;
    bool admissible = false;   // the fp32 screen may run
    bool prune = false;        // launch the pruning variant (pruning_pays)
    bool screen = false;       // launch the fp32-screen variant (screen_pays)
};
inline FluxChoice choose_flux_kernels(const SearchPlan& plan, const Switches& opt, const std::vector<tlsdev::WidthEntry>& widths,
                                      double sigma, double depth_min, bool screen_admits, bool prune_beside_screen = true) {
    FluxChoice f;
    f.sigma = sigma;
    f.admissible = screen_admits && !plan.short_rows;   // (neither variant forms a short row's tail term: the plain kernel, switches or not)
    f.prune = plan.uniform && !plan.short_rows && pruning_pays(opt, widths, sigma, depth_min, plan.resident, prune_beside_screen && f.admissible);
    f.screen = screen_pays(opt, widths, sigma, depth_min, f.admissible);
    return f;
}

// The kernel families a search launches; the names are what tls_last_kernel reports.
enum class Kernel { Slim, Slim512, Resident, ResidentPrune, ResidentScreen, Slab, SlabSplit };
inline const char* kernel_name(Kernel k) {
    switch (k) {
        case Kernel::Slim: return "slim";
        case Kernel::Slim512: return "slim512";
        case Kernel::Resident: return "resident";
        case Kernel::ResidentPrune: return "resident+prune";
        case Kernel::ResidentScreen: return "resident+screen32";
        case Kernel::Slab: return "slab";
        case Kernel::SlabSplit: return "slab+split";
    }
    return "";
}
inline bool is_slim(Kernel k) { return k == Kernel::Slim || k == Kernel::Slim512; }

// what one launch adds to the plan and the flux: a plain search sets none of them
struct LaunchFlags {
    bool count_work = false;    // the counting instantiation (it evaluates every cell: no pruning, no screen)
    bool debug_entry = false;   // debug_folded / debug_prefix: the plain classic (or slab) kernel
    int batch_curves = 1;       // light curves of the launch (tls_search_batch); the two roles search one
};
inline Kernel pick_kernel(const SearchPlan& plan, const FluxChoice& flux, const LaunchFlags& launch = LaunchFlags()) {
    // pruning variant: LDS-resident series, uniform weights, noisy enough that most trial cells pass the depth predicate,
    // and not while the evaluated cells are being counted (counting means evaluating all of them)
    const bool prune = plan.resident && plan.uniform && flux.prune && !launch.count_work;
    // fp32 screen of the dot products (tlsdev::screen_cells): where the host expects it to pay (screen_pays); counting the
    // work and the debug entries run the plain variant, whose bits it returns anyway
    const bool screen_chosen = flux.screen && flux.admissible;
    if (screen_chosen && !prune && !launch.count_work && !launch.debug_entry) return Kernel::ResidentScreen;
    // Four period slots per CU (tls_slim_kernel.hip.h): plain variant, uniform weights.  By the plan's choice, not this
    // launch's: a search that counts its work runs the counting instantiation of the kernel the plain search takes -- the
    // classic family where pruning or the screen is the host's choice -- and returns its bits.
    if (plan.slim_blocks > 0 && plan.uniform && !flux.prune && !screen_chosen && !launch.debug_entry)
        return plan.slim_threads == tlsdev::kSlimThreadsWide ? Kernel::Slim512 : Kernel::Slim;
    if (plan.resident) return prune ? Kernel::ResidentPrune : Kernel::Resident;
    return plan.split && launch.batch_curves == 1 ? Kernel::SlabSplit : Kernel::Slab;
}

}  // namespace tlsplan
