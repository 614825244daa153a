// tls_amd.hip -- host side of libtls_amd.so: the C ABI of include/tls_amd.h.
//
// Builds the device work list for one light curve (distinct trial widths, per-period
// duration windows, cost-ordered period queue), keeps every buffer resident in HBM between
// calls, launches the search kernel of tls_kernels.hip.h and gathers results; optional RCCL
// all-gather for the period-sharded multi-GPU mode.
//
// Reference mapping: main.py:140-196 (dispatch + ordered gather), core.py:113-116,143-156
// (width list, duration window per period), grid.py:9-32 (T14).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include "../../include/tls_amd.h"
#include "tls_kernels.hip.h"
#include "tls_plan.hip.h"
#include "tls_candidate_slabs.h"
#include "tls_arena.h"

// every DevBuf is device memory of the HIP runtime (a hipError_t travels as the int it is)
int tlsmem::device_alloc(void** out, size_t bytes) { return (int)hipMalloc(out, bytes); }
int tlsmem::device_free(void* p) { return (int)hipFree(p); }

using namespace tlsplan;

namespace {

constexpr size_t kEventRing = 64;   // launch-timing event pairs kept per context
// what a new context's switch `lanes` starts as (A/B builds: make variant NAME=nolanes DEFS=-DTLS_LANES_DEFAULT=0 runs an
// unchanged bench.py with every launch on lane A)
#ifndef TLS_LANES_DEFAULT
#define TLS_LANES_DEFAULT -1
#endif

std::string g_create_error;  // tls_last_error(NULL)

using tlsmem::Arena;
using tlsmem::BufPool;
using tlsmem::DevBuf;
constexpr tlsmem::Kind kScratch = tlsmem::Kind::scratch, kState = tlsmem::Kind::state;

// a typed window into the context's one plan allocation (d_plan): same `.ptr` as a DevBuf, not owned
template <typename T>
struct View {
    T* ptr = nullptr;
};

struct SwitchName { const char* name; const char* env; size_t offset; int kind; };   // kind 0: int32, 1: int64, 2: double
#define TLS_SW(field, env, kind) { #field, env, offsetof(Switches, field), kind }
const SwitchName kSwitchNames[] = {
    TLS_SW(exact_prefix, "TLS_EXACT_PREFIX", 0), TLS_SW(slim, "TLS_SLIM", 0), TLS_SW(prune, "TLS_PRUNE", 0),
    TLS_SW(screen32, "TLS_SCREEN32", 0), TLS_SW(no_screen, "TLS_NO_SCREEN", 0), TLS_SW(fast_slab, "TLS_FAST_SLAB", 0),
    TLS_SW(x_staged, "TLS_X_STAGED", 0), TLS_SW(split, "TLS_SPLIT", 0), TLS_SW(split_batch, "TLS_SPLIT_BATCH", 0),
    TLS_SW(sort2, "TLS_SORT2", 0), TLS_SW(threads, "TLS_THREADS", 0), TLS_SW(blocks, "TLS_BLOCKS", 0),
    TLS_SW(plan_threads, "TLS_PLAN_THREADS", 0), TLS_SW(t0_rot, "TLS_T0_ROT", 0), TLS_SW(prune_min_live, "TLS_PRUNE_MIN_LIVE", 1),
    TLS_SW(perm_table, "TLS_PERM_TABLE", 1), TLS_SW(reg_scan, "TLS_REG_SCAN", 0),
    TLS_SW(dense_hoist, "TLS_DENSE_HOIST", 0), TLS_SW(claim_ahead, "TLS_CLAIM_AHEAD", 0),
    TLS_SW(band_max, "TLS_BAND_MAX", 2),
};
#undef TLS_SW
const SwitchName* find_switch(const char* name) {
    for (const auto& sw : kSwitchNames) if (name && std::strcmp(sw.name, name) == 0) return &sw;
    return nullptr;
}
void switch_store(Switches& o, const SwitchName& sw, double value) {
    unsigned char* at = reinterpret_cast<unsigned char*>(&o) + sw.offset;
    if (sw.kind == 0) { const int32_t v = value < 0 ? -1 : (int32_t)value; std::memcpy(at, &v, sizeof v); }
    else if (sw.kind == 1) { const int64_t v = value < 0 ? -1 : (int64_t)value; std::memcpy(at, &v, sizeof v); }
    else { const double v = value < 0 ? -1.0 : value; std::memcpy(at, &v, sizeof v); }
}
double switch_load(const Switches& o, const SwitchName& sw) {
    const unsigned char* at = reinterpret_cast<const unsigned char*>(&o) + sw.offset;
    if (sw.kind == 0) { int32_t v; std::memcpy(&v, at, sizeof v); return (double)v; }
    if (sw.kind == 1) { int64_t v; std::memcpy(&v, at, sizeof v); return (double)v; }
    double v; std::memcpy(&v, at, sizeof v); return v;
}
// every switch "the library decides" (all bytes defined: plans are keyed by memcmp over the struct)
Switches default_switches() {
    Switches o;
    std::memset(&o, 0, sizeof o);
    for (const auto& sw : kSwitchNames) switch_store(o, sw, -1.0);
    return o;
}
// "name=value,name=value" (what tls_debug_get_switches writes) over a set of switches; false on an unknown name
bool switches_parse(Switches& o, const char* spec) {
    if (!spec) return true;
    std::string text(spec);
    size_t at = 0;
    while (at < text.size()) {
        size_t end = text.find(',', at);
        if (end == std::string::npos) end = text.size();
        const std::string item = text.substr(at, end - at);
        at = end + 1;
        if (item.empty()) continue;
        const size_t eq = item.find('=');
        if (eq == std::string::npos) return false;
        const SwitchName* sw = find_switch(item.substr(0, eq).c_str());
        if (!sw) return false;
        switch_store(o, *sw, std::atof(item.c_str() + eq + 1));
    }
    return true;
}

// The TLS_* environment variables (one per switch, kSwitchNames), read ONCE per process: what a new context starts with and
// what the context-free planning call (tls_period_costs) uses when it is given no switches.  Nothing reads the environment
// after this.
const Switches& process_options() {
    static const Switches cached = [] {
        Switches o = default_switches();
        for (const auto& sw : kSwitchNames)
            if (const char* v = std::getenv(sw.env)) switch_store(o, sw, (*v == 0 && sw.kind == 0) ? 1.0 : std::atof(v));
        return o;
    }();
    return cached;
}

// what a prepared plan was built from: a second tls_prepare with the same time stamps, period list, template table,
// parameters and developer switches only replaces the flux (the search call of a survey, or of repeated power()
// calls).  Compared byte for byte (memcmp runs at ~10 GB/s; a cfg2 key is 120 KB).
struct PlanLayout {   // byte offsets of the plan arrays inside d_plan / h_stage (256-byte aligned)
    size_t t = 0, y = 0, w = 0, periods = 0, order = 0, rows = 0, widths = 0, screens = 0, q = 0, q2 = 0, g = 0, tile_prefix = 0, total = 0;
};

struct PlanKey {
    bool valid = false;
    int64_t n = 0, n_periods = 0, n_rows = 0;
    std::vector<double> t, periods, values, overshoot;
    std::vector<int64_t> offset, length, width;
    tls_params params = {0, 0, 0, 0, 0, 0};
    Switches opt;
};

// Lane B of a context (tls_ctx::lane_b; DESIGN.md section 4, "Launch lanes"): a second stream and a second set of exactly
// what an overlappable four-slot launch writes, and of the flux.  Allocated at lane B's first use.
struct LaneB {
    explicit LaneB(BufPool& owner) : pool(owner) {}
    BufPool& pool;                        // the context's
    hipStream_t stream = nullptr;
    DevBuf<unsigned int> d_squeue{pool, "lane_b.d_squeue", kState};   // state: a queue whose zero state between launches is the kernels' own invariant
    // (smeared on the joined stream, which lane B's next command waits for)
    DevBuf<unsigned int> d_lists{pool, "lane_b.d_lists", kScratch}, d_perm{pool, "lane_b.d_perm", kScratch};
    // [chi2 | row | depth | counters[4]]; the flux.  State: results a later call may trust; the flux the next launch reads
    DevBuf<double> d_out{pool, "lane_b.d_out", kState}, d_y{pool, "lane_b.d_y", kState};
    unsigned char* h_stage = nullptr; size_t h_stage_cap = 0;   // pinned: the flux on its way to d_y
    hipEvent_t ev_stage = nullptr; bool stage_pending = false;   // ... and its last upload
    hipEvent_t ev_done = nullptr;         // behind the last command on `stream` (launch or upload)
    bool outstanding = false;             // ev_done is recorded and lane A has not waited for it
    bool saw_state = false;               // `stream` has waited for the latest record of ev_state
};

}  // namespace

struct tls_ctx {
    int device = 0;
    // Every device buffer of the context is constructed against this pool (lane B's and the batch slots' too), with its name
    // and kind (DESIGN.md "Device memory"): tls_ctx_destroy, tls_debug_device_bytes and tls_debug_poison_lds walk the pool.
    // scratch: the next call uploads or writes all that it reads from the buffer; state: the one-line reason beside it.
    BufPool pool;
    // Lane A's stream: the context's one stream for everything but a lane-B launch and its flux.  Every use outside the
    // lane path goes through main_stream(ctx), which first orders the stream behind lane B (join) -- hence the name no
    // other code spells.
    hipStream_t lane_a_stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // Launch lanes: back-to-back plain four-slot searches of a plan whose table of folded orders is
    // filled alternate between lane A (the buffers below, as ever) and lane B -- a second stream and a second set of
    // exactly what such a launch writes (queue words, live-unit lists with the band list, stashed orders, results) and of
    // the flux --, so that search i+1 starts on the compute units search i has already left.  Lane B's buffers are
    // allocated at its first use (a context that never overlaps holds none of them).
    LaneB lane_b{pool};
    hipEvent_t ev_state = nullptr;            // lane A's state a lane-B command must see: uploads, the filling launch, consumers
    bool state_dirty = true;                  // lane A's stream got a command other than an overlapped launch since ev_state's record
    int lanes = TLS_LANES_DEFAULT;            // developer switch `lanes` (0: every launch on lane A); not part of the plan key
    int run_lane = -1;                        // lane of the previous launch if it was an overlappable one and nothing but tls_update_flux came since; else -1
    int result_lane = 0;                      // lane whose results d_latest / d_chi2 / d_row / d_depth / d_counters denote: the LATEST launch's
    int flux_lane = 0;                        // lane whose flux buffer d_y denotes: the flux of the NEXT launch
    bool flux_b_unseen = false;               // lane B's flux was uploaded and lane A's stream has not waited for that
    bool a_reads_flux_b = false, b_reads_flux_a = false;   // a launch read the OTHER lane's flux, and that lane's stream is not yet ordered behind it
    bool perm_filled_before_prev = false;     // perm_filled as the previous launch found it
    int64_t lane_launches[2] = {0, 0};        // launches sent to each lane (tls_debug_lanes)
    View<double> d_y_a;                       // lane A's flux (inside d_plan)
    std::string err;
    std::string name;
    int n_cu = 0;

    // device-resident plan
    // ONE allocation holds every plan array (views below); it is filled from ONE pinned staging buffer by ONE
    // asynchronous copy, and tls_prepare does not wait for it
    DevBuf<unsigned char> d_plan{pool, "d_plan", kState};   // state: the plan
    View<double> d_t, d_y, d_w, d_periods, d_q, d_q2, d_g;
    View<int> d_order;
    View<tlsdev::PeriodRows> d_rows;
    View<tlsdev::WidthEntry> d_widths;
    View<tlsdev::RowScreen> d_screens;
    unsigned char* h_stage = nullptr; size_t h_stage_cap = 0;   // pinned: the plan (tls_prepare) / the flux (tls_update_flux)
    hipEvent_t ev_stage = nullptr; bool stage_pending = false;  // its last upload
    // results: [chi2 | row | depth | counters[4]] in one allocation, fetched by one copy into pinned memory.  d_out is
    // lane A's allocation; the views denote the results of the LATEST launch, whichever lane it took (point_results)
    DevBuf<double> d_out{pool, "d_out", kState};   // state: results a later call may trust (tls_spectra without chi2)
    View<double> d_latest;
    View<double> d_chi2, d_depth;
    View<long long> d_row;
    View<unsigned long long> d_counters;
    double* h_out = nullptr; size_t h_out_cap = 0;
    PlanKey key;
    PlanLayout layout;
    int64_t plan_reuses = 0;   // tls_prepare calls answered from the held plan
    std::vector<double> batch_group_ms;   // wall time of every group of 32 light curves of the last tls_power_batch / tls_search_batch (tls_debug_batch_group_ms)
    std::vector<double> batch_group_wait_ms;   // ... of which the group's one wait for the device (tls_power_batch)
    DevBuf<double> d_scratch{pool, "d_scratch", kScratch}, d_pack{pool, "d_pack", kScratch}, d_scalar{pool, "d_scalar", kScratch};
    // state: the staged / gathered results of the comm calls, which a later call may trust
    DevBuf<double> d_gather{pool, "d_gather", kState}, d_stage{pool, "d_stage", kState};
    // state: queues and counters whose zero state between launches is the kernels' own invariant
    DevBuf<unsigned long long> d_phase{pool, "d_phase", kState}, d_check{pool, "d_check", kState};
    DevBuf<unsigned int> d_queue{pool, "d_queue", kState};
    DevBuf<unsigned int> d_squeue{pool, "d_squeue", kState};     // the search kernel's self-rewinding queue
    DevBuf<unsigned int> d_pqueues{pool, "d_pqueues", kState};   // tls_power_batch's T0-fit queues
    DevBuf<unsigned int> d_lists{pool, "d_lists", kScratch}, d_perm{pool, "d_perm", kScratch};
    // state: inputs of the survey batches
    DevBuf<double> d_curve_S0{pool, "d_curve_S0", kState}, d_curve_w0{pool, "d_curve_w0", kState};
    // The four-slot kernel's table of folded orders: one row per period of the plan (tlsdev::slim_perm_row entries).  The
    // order is numpy's stable argsort of fold_phase(t, period) -- the flux, the weights and the noise do not enter it --, so
    // it lives as long as the plan key: the plan's first four-slot launch stores it, every later one reads it.
    // state: it belongs to the plan (grows like every DevBuf and is kept: plans of different period counts alternate on a context)
    DevBuf<unsigned short> d_perm_table{pool, "d_perm_table", kState};
    size_t perm_table_entries = 0;           // entries of it the held plan uses; 0: the plan has no table
    bool perm_filled = false;                // a launch that stored every row has been enqueued (stream order does the rest)
    // survey batches: two slots of device + pinned host buffers, a second stream for the transfers
    struct BatchSlot {
        explicit BatchSlot(BufPool& owner) : pool(owner) {}
        BufPool& pool;                                   // the context's
        // state: the inputs and results of the survey batches
        DevBuf<double> d_y{pool, "slot.d_y", kState}, d_w{pool, "slot.d_w", kState}, d_S0{pool, "slot.d_S0", kState},
            d_w0{pool, "slot.d_w0", kState}, d_chi2{pool, "slot.d_chi2", kState}, d_depth{pool, "slot.d_depth", kState};
        DevBuf<long long> d_row{pool, "slot.d_row", kState};
        double* h_in = nullptr; size_t h_in_cap = 0;     // pinned: y | w | S0 | w0 of one group
        double* h_out = nullptr; size_t h_out_cap = 0;   // pinned: chi2 | row | depth of one group
        hipEvent_t ev_in = nullptr, ev_kernel = nullptr, ev_out = nullptr;
    } slot[2] = {BatchSlot(pool), BatchSlot(pool)};
    hipStream_t copy_stream = nullptr;
    // enqueue() reads these when set (a batch slot); otherwise the context's own buffers
    const double* over_y = nullptr; const double* over_w = nullptr;
    const double* over_S0 = nullptr; const double* over_w0 = nullptr;
    double* over_chi2 = nullptr; long long* over_row = nullptr; double* over_depth = nullptr;
    int batch_curves = 1;                    // light curves the next launch searches (tls_search_batch)
    // the final T0 fit
    DevBuf<double> d_ft{pool, "d_ft", kScratch}, d_fy{pool, "d_fy", kScratch}, d_fsig{pool, "d_fsig", kScratch}, d_fep{pool, "d_fep", kScratch},
        d_fres{pool, "d_fres", kScratch}, d_fscratch{pool, "d_fscratch", kScratch};
    DevBuf<double> d_pink{pool, "d_pink", kScratch};          // tls_pink_noise
    DevBuf<double> d_frot{pool, "d_frot", kScratch};          // the T0 fit's rotation path: per fit flux, phases, quotients of the base order, state
    DevBuf<int> d_frperm{pool, "d_frperm", kScratch};         // ... and the base order itself
    DevBuf<double> d_spec{pool, "d_spec", kScratch};          // the SDE spectra and what tls_power_batch copies out of a group
    DevBuf<double> d_tstats{pool, "d_tstats", kScratch};      // tls_power_batch_stats: the tables and the per-curve scratch of one group
    DevBuf<int> d_tranges{pool, "d_tranges", kScratch};       // ... and every epoch's chunk start | stop | offset
    DevBuf<double> d_models{pool, "d_models", kScratch};      // tls_power_batch_models
    DevBuf<double> d_inject{pool, "d_inject", kScratch};      // tls_inject_transits
    DevBuf<unsigned long long> d_inject_count{pool, "d_inject_count", kScratch};   // ... and its points in contact per injection
    DevBuf<double> d_null{pool, "d_null", kScratch};          // tls_null_rows
    DevBuf<unsigned long long> d_null_words{pool, "d_null_words", kScratch};       // tls_debug_null_words: the words of one slab
    DevBuf<double> d_detrend{pool, "d_detrend", kScratch};    // tls_medfilt_detrend, tls_biweight_detrend: the rows of one slab
    DevBuf<int> d_windows{pool, "d_windows", kScratch};       // tls_biweight_detrend: the window of every point
    // tls_transit_mask, tls_biweight_detrend_masked, tls_remove_transits: time stamps, grouped candidates, rows of one slab
    DevBuf<double> d_protect{pool, "d_protect", kScratch};
    // ... and their mask rows of one slab (tls_prewhiten_masked's too)
    DevBuf<unsigned char> d_protect_bytes{pool, "d_protect_bytes", kScratch};
    DevBuf<double> d_sysrem{pool, "d_sysrem", kScratch};      // tls_sysrem
    // ... and its state words (tlsdev::kSysremState).  State: counters whose zero state between launches is the kernels' own invariant
    DevBuf<unsigned long long> d_sysrem_state{pool, "d_sysrem_state", kState};
    DevBuf<double> d_peaks{pool, "d_peaks", kScratch};        // tls_find_peaks
    DevBuf<unsigned long long> d_peak_mask{pool, "d_peak_mask", kScratch};   // ... and tls_power_batch_peaks: a row's alive mask where the LDS does not hold it
    // the peak-fit stage (tls_power_batch_peak_fits), one slab of fits: inputs and fit records; trial epochs; residuals; the
    // statistics kernel's scratch and its chunk ranges
    DevBuf<double> d_pfit{pool, "d_pfit", kScratch}, d_pfep{pool, "d_pfep", kScratch}, d_pfres{pool, "d_pfres", kScratch},
        d_pfstats{pool, "d_pfstats", kScratch};
    DevBuf<int> d_pfranges{pool, "d_pfranges", kScratch};
    DevBuf<double> d_scan{pool, "d_scan", kScratch};          // tls_phase_scan
    DevBuf<double> d_single{pool, "d_single", kScratch};      // tls_single_transits
    // the per-candidate stages (run_candidate_slabs): one slab's curve rows and per-candidate arrays, then what every slab shares
    DevBuf<double> d_times{pool, "d_times", kScratch};        // tls_transit_times
    DevBuf<double> d_vetting{pool, "d_vetting", kScratch};    // tls_event_vetting
    DevBuf<double> d_shape{pool, "d_shape", kScratch};        // tls_shape_fit
    DevBuf<double> d_transit{pool, "d_transit", kScratch};    // tls_transit_fit
    DevBuf<double> d_centroid{pool, "d_centroid", kScratch};  // tls_centroid_test
    DevBuf<double> d_views{pool, "d_views", kScratch};        // tls_folded_views
    DevBuf<double> d_gls{pool, "d_gls", kScratch};            // tls_nudft, tls_lomb_scargle, tls_sine_test, prewhiten
    DevBuf<double> d_match{pool, "d_match", kScratch};        // tls_ephemeris_match
    DevBuf<double> d_noise{pool, "d_noise", kScratch};        // tls_noise_profile
    DevBuf<double> d_aliases{pool, "d_aliases", kScratch};    // tls_event_periods
    DevBuf<double> d_decor{pool, "d_decor", kScratch};        // tls_decorrelate
    DevBuf<double> d_spline{pool, "d_spline", kScratch};      // tls_spline_detrend
    DevBuf<double> d_clean{pool, "d_clean", kScratch};        // tls_clean_rows
    // two-role slab path (series in HBM, one light curve; SearchPlan::split)
    View<unsigned int> d_tile_prefix;        // [n_periods + 1] tiles in front of work item w (queue order)
    DevBuf<double> d_partials{pool, "d_partials", kScratch};  // [split_max_items][3] a tile's winner
    // [split_batch] tiles of the period that are done.  State: zero between launches is the kernels' own invariant
    DevBuf<unsigned int> d_tiles_done{pool, "d_tiles_done", kState};
    std::vector<tlsdev::WidthEntry> host_widths;  // kept for tls_update_flux's pruning decision
    Switches opt;                     // the context's switches (tls_set_options / tls_debug_set_switch; initially the process's TLS_* environment)

    // host-side plan
    bool prepared = false, executed = false;
    SearchPlan plan;                 // what tls_prepare decided (plan_search): sizes, launch shapes, the slab's tiles
    FluxChoice flux;                 // ... and what the flux of the next launch adds (choose_flux_kernels)
    const char* last_kernel = "";    // tls_last_kernel
    double S0 = 0, w0 = 1, depth_min = 0;
    double y_abs_max = 1.0;   // largest |flux| of the light curve(s) of the next launch: bounds the prefix sum (fast mode's eps)
    double e_abs_max = INFINITY;   // largest |1 - flux| of the same (inf: a sample outside [0.5, 2]): admits the fp32 screen
    DevBuf<float> d_split{pool, "d_split", kScratch};    // fp32 screen: low halves of the folded samples, one region per workgroup
    DevBuf<double> d_park{pool, "d_park", kScratch};     // fp32 screen: parked cells, kParkCap per workgroup
    // slab variant, fast mode: band_prefix of the launches (two slots, like h_band).  State: the host caches it by sigma
    DevBuf<double> d_band{pool, "d_band", kState};
    double* d_band_now = nullptr;   // the slot the next launch reads
    double* h_band = nullptr; size_t h_band_cap = 0;   // pinned: two slots of (n_widths + 1) doubles
    hipEvent_t ev_band[2] = {nullptr, nullptr}; bool band_used[2] = {false, false}; int band_slot = 0;
    double band_sigma = -1.0, band_eps = -1.0;   // what d_band was computed for
    long long q_count = 0;    // elements of the padded template rows (the fp32 screen's second copy starts there)
    tls_counters plan_counters = {0, 0, 0, 0, 0};
    bool counted = false;

    // per-launch kernel timing (HIP events on the launch's stream)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    std::vector<char> ev_overlapped;   // [ring slot] the launch may have begun before the one in the slot before it ended
    size_t ev_used = 0;

    // RCCL
    ncclComm_t comm = nullptr;
    int n_ranks = 1, rank = 0;
    int64_t gathered_count = 0;
};

namespace {

int update_flux_impl(tls_ctx* ctx, const double* y, const double* dy);
constexpr int kWeightsDiffer = 1;

int fail(tls_ctx* ctx, int code, const std::string& msg) {
    if (ctx) ctx->err = msg; else g_create_error = msg;
    return code;
}

#define TLS_HIP(ctx, call)                                                              \
    do {                                                                                \
        hipError_t e_ = static_cast<hipError_t>(call);                                                \
        if (e_ != hipSuccess)                                                           \
            return fail(ctx, TLS_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

#define TLS_NCCL(ctx, call)                                                             \
    do {                                                                                \
        ncclResult_t r_ = (call);                                                       \
        if (r_ != ncclSuccess)                                                          \
            return fail(ctx, TLS_E_RCCL, std::string(#call) + ": " + ncclGetErrorString(r_)); \
    } while (0)

// ---- launch lanes: ordering -------------------------------------------------------------------------------------------
// Every wait names an event recorded EARLIER in host order, so the dependencies form a DAG: nothing can wait on itself.

// lane A's stream ordered behind everything lane B has been given; costs nothing when lane B has nothing outstanding
void lanes_join(tls_ctx* ctx) {
    auto& lb = ctx->lane_b;
    if (lb.outstanding) {
        if (hipStreamWaitEvent(ctx->lane_a_stream, lb.ev_done, 0) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipStreamSynchronize(lb.stream);   // (the host waits instead: always right)
        }
        lb.outstanding = false;
    }
    ctx->flux_b_unseen = false; ctx->b_reads_flux_a = false;
}

// The context's stream for every command outside the lane path: joined, and the command that follows ends the run of
// overlappable launches (the next search takes lane A) and is something lane B's next command has to see.
hipStream_t main_stream(tls_ctx* ctx) {
    lanes_join(ctx);
    ctx->run_lane = -1;
    ctx->state_dirty = true;
    return ctx->lane_a_stream;
}

// the results the views denote: those of `lane`
void point_results(tls_ctx* ctx, int lane) {
    double* base = lane ? ctx->lane_b.d_out.ptr : ctx->d_out.ptr;
    const size_t np = (size_t)ctx->plan.n_periods;
    ctx->d_latest.ptr = base;
    ctx->d_chi2.ptr = base; ctx->d_row.ptr = reinterpret_cast<long long*>(base + np);
    ctx->d_depth.ptr = base + 2 * np;
    ctx->d_counters.ptr = reinterpret_cast<unsigned long long*>(base + 3 * np);
    ctx->result_lane = lane;
}

// the pinned staging buffer, at least `bytes` long and no longer read by an upload in flight
int stage_reserve(tls_ctx* ctx, size_t bytes) {
    if (!ctx->ev_stage) TLS_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_stage, hipEventDisableTiming));
    if (ctx->stage_pending) { TLS_HIP(ctx, hipEventSynchronize(ctx->ev_stage)); ctx->stage_pending = false; }
    if (ctx->h_stage_cap < bytes) {
        if (ctx->h_stage) TLS_HIP(ctx, hipHostFree(ctx->h_stage));
        ctx->h_stage = nullptr; ctx->h_stage_cap = 0;
        const size_t cap = std::max<size_t>(bytes + bytes / 4, 1 << 16);
        TLS_HIP(ctx, hipHostMalloc(reinterpret_cast<void**>(&ctx->h_stage), cap, hipHostMallocDefault));
        ctx->h_stage_cap = cap;
    }
    return TLS_OK;
}

// the bound-check counters (tls_debug_check_counts): allocated and zeroed on first use
int ensure_check_counters(tls_ctx* ctx) {
    if (ctx->d_check.ptr) return TLS_OK;
    TLS_HIP(ctx, ctx->d_check.reserve(tlsdev::kChecks));
    TLS_HIP(ctx, hipMemsetAsync(ctx->d_check.ptr, 0, tlsdev::kChecks * sizeof(unsigned long long), main_stream(ctx)));
    return TLS_OK;
}

// ---- argument checks the survey stages share; `what` ("transit times") starts every message
int check_batch(tls_ctx* ctx, const std::string& what, int64_t n, int64_t n_max, const char* range_text, int64_t n_fits,
                int64_t n_curves) {
    if (n < 1 || n > n_max) return fail(ctx, TLS_E_ARG, what + ": n out of range " + range_text);
    if (n_fits > INT32_MAX || (uint64_t)n_curves > (uint64_t)(INT64_MAX / 16) / (uint64_t)n)
        return fail(ctx, TLS_E_ARG, what + ": batch too large");
    return TLS_OK;
}

int check_time_stamps(tls_ctx* ctx, const std::string& what, const double* t, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(t[i]) || (i > 0 && t[i] < t[i - 1]))
            return fail(ctx, TLS_E_ARG, what + ": the time stamps must be finite and non-decreasing");
    return TLS_OK;
}

// curve null: candidate f reads curve f; more(f): what else a stage asks of candidate f, checked behind its curve
template <typename More>
int check_curves(tls_ctx* ctx, const std::string& what, const int64_t* curve, int64_t n_fits, int64_t n_curves, More more) {
    for (int64_t f = 0; f < n_fits; ++f) {
        const int64_t c = curve ? curve[f] : f;
        if (c < 0 || c >= n_curves) return fail(ctx, TLS_E_ARG, what + ": curve out of range [0, n_curves)");
        if (int rc = more(f)) return rc;
    }
    return TLS_OK;
}
int check_curves(tls_ctx* ctx, const std::string& what, const int64_t* curve, int64_t n_fits, int64_t n_curves) {
    return check_curves(ctx, what, curve, n_fits, n_curves, [](int64_t) { return TLS_OK; });
}

size_t template_values(const tls_template* tmpl) {
    int64_t total = 0;
    for (int64_t r = 0; r < tmpl->n_rows; ++r) total = std::max(total, tmpl->offset[r] + std::max<int64_t>(tmpl->length[r], 0));
    return (size_t)std::max<int64_t>(total, 0);
}

bool key_matches(const PlanKey& k, const Switches& opt, const double* t, int64_t n, const double* periods, int64_t n_periods,
                 const tls_template* tmpl, const tls_params* params) {
    if (!k.valid || k.n != n || k.n_periods != n_periods || k.n_rows != tmpl->n_rows) return false;
    if (std::memcmp(&k.params, params, sizeof(tls_params)) != 0) return false;
    const size_t rows = (size_t)tmpl->n_rows;
    if (std::memcmp(k.offset.data(), tmpl->offset, rows * 8) || std::memcmp(k.length.data(), tmpl->length, rows * 8) ||
        std::memcmp(k.width.data(), tmpl->width, rows * 8) || std::memcmp(k.overshoot.data(), tmpl->overshoot, rows * 8))
        return false;
    if (k.values.size() != template_values(tmpl) || std::memcmp(k.values.data(), tmpl->values, k.values.size() * 8)) return false;
    if (std::memcmp(k.t.data(), t, (size_t)n * 8) || std::memcmp(k.periods.data(), periods, (size_t)n_periods * 8)) return false;
    return std::memcmp(&k.opt, &opt, sizeof(Switches)) == 0;
}

void key_store(PlanKey& k, const Switches& opt, const double* t, int64_t n, const double* periods, int64_t n_periods,
               const tls_template* tmpl, const tls_params* params) {
    k.n = n; k.n_periods = n_periods; k.n_rows = tmpl->n_rows; k.params = *params;
    k.t.assign(t, t + n); k.periods.assign(periods, periods + n_periods);
    const size_t rows = (size_t)tmpl->n_rows;
    k.offset.assign(tmpl->offset, tmpl->offset + rows); k.length.assign(tmpl->length, tmpl->length + rows);
    k.width.assign(tmpl->width, tmpl->width + rows); k.overshoot.assign(tmpl->overshoot, tmpl->overshoot + rows);
    k.values.assign(tmpl->values, tmpl->values + template_values(tmpl));
    k.opt = opt;
    k.valid = true;
}

template <typename T>
int upload(tls_ctx* ctx, DevBuf<T>& buf, const T* host, size_t count) {
    TLS_HIP(ctx, buf.reserve(count));
    if (count)
        TLS_HIP(ctx, hipMemcpyAsync(buf.ptr, host, count * sizeof(T), hipMemcpyHostToDevice, main_stream(ctx)));
    return TLS_OK;
}

// weights and the period-independent constant S0 = sum (1-y)^2 / dy^2
void weights_from(const double* y, const double* dy, int64_t n, bool& uniform, double& w0,
                  std::vector<double>& w, double& S0, double* y_abs_max = nullptr, double* e_abs_max = nullptr) {
    if (y_abs_max) {
        double m = 0.0;
        for (int64_t i = 0; i < n; ++i) m = std::max(m, std::fabs(y[i]));
        *y_abs_max = std::max(*y_abs_max, m);
    }
    if (e_abs_max) {
        // 1 - y is exact for y in [0.5, 2] (Sterbenz) and a multiple of 2^-53 there: what the fp32 screen's split needs
        double m = 0.0;
        for (int64_t i = 0; i < n; ++i) m = (y[i] >= 0.5 && y[i] <= 2.0) ? std::max(m, std::fabs(1 - y[i])) : INFINITY;
        *e_abs_max = std::max(*e_abs_max, m);
    }
    uniform = true;
    for (int64_t i = 1; i < n; ++i)
        if (dy[i] != dy[0]) { uniform = false; break; }
    long double acc = 0.0L;
    if (uniform) {
        w0 = 1 / (dy[0] * dy[0]);  // core.py:127
        w.clear();
        for (int64_t i = 0; i < n; ++i) acc += (long double)((1 - y[i]) * (1 - y[i])) * w0;
    } else {
        w0 = 1.0;
        w.resize((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
            w[(size_t)i] = 1 / (dy[i] * dy[i]);
            acc += (long double)((1 - y[i]) * (1 - y[i])) * w[(size_t)i];
        }
    }
    S0 = (double)acc;
}

// Distinct trial widths ascending with the first template row of each (core.py:113,163-165),
// their T0 stride (core.py:50-55) and, optionally, the q_j = 1 - signal_j rows.
int build_widths(tls_ctx* ctx, const tls_template* tmpl, const tls_params* params, int64_t n,
                 std::vector<tlsdev::WidthEntry>& widths, std::vector<double>* q) {
    if (!tmpl || !params) return fail(ctx, TLS_E_ARG, "null argument");
    if (tmpl->n_rows < 1 || !tmpl->values || !tmpl->offset || !tmpl->length || !tmpl->width || !tmpl->overshoot)
        return fail(ctx, TLS_E_ARG, "empty template table");
    std::vector<int64_t> rows((size_t)tmpl->n_rows);
    std::iota(rows.begin(), rows.end(), 0);
    std::stable_sort(rows.begin(), rows.end(), [&](int64_t a, int64_t b) { return tmpl->width[a] < tmpl->width[b]; });
    const double margin = params->T0_fit_margin;
    size_t q_count = 0;
    for (int64_t r : rows) {
        const int64_t wd = tmpl->width[r];
        if (!widths.empty() && widths.back().width == wd) continue;  // later duplicates never used
        if (wd < 1 || wd > n) return fail(ctx, TLS_E_ARG, "template width out of range [1, n]");
        const int64_t len = tmpl->length[r];
        if (len < 1 || len > wd) return fail(ctx, TLS_E_ARG, "template row longer than its width");
        tlsdev::WidthEntry we;
        we.width = (int)wd; we.row = (int)r; we.q_len = (int)len;
        we.n_pos = 0; we.n_chunks = 0; we.list_base = 0; we.inv_d = 1.0 / (double)wd;
        we.xth = 1;
        if (margin > 0 && (double)wd > margin) {  // core.py:50-55
            const double inv = 1 / margin;
            int xth = (int)((double)wd / inv);
            we.xth = xth < 1 ? 1 : xth;
        }
        we.tiled = tlsdev::row_is_tiled(we.width, we.xth) ? 1 : 0;
        we.oversize = 0; we.pad_ = 0;
        // rows are stored zero padded (pad_front before, pad_back after, then up to a multiple
        // of 8 doubles) so that the unrolled dot product needs no edge handling; the pads grow
        // with the stride of a tiled row (its kR windows reach (kR-1)*xth samples further)
        const size_t front = (size_t)tlsdev::pad_front(we.tiled ? we.xth : 1);
        const size_t back = (size_t)tlsdev::pad_back(we.tiled ? we.xth : 1);
        we.q_offset = (int)(q_count + front);
        we.overshoot = tmpl->overshoot[r];
        double s2 = 0.0, s1 = 0.0, s_abs = 0.0;
        if (q) q->insert(q->end(), front, 0.0);
        for (int64_t j = 0; j < len; ++j) {
            const double qj = 1 - tmpl->values[tmpl->offset[r] + j];  // core.py:68
            if (q) q->push_back(qj);
            s2 += qj * qj;
            s1 += qj;
            s_abs += std::fabs(qj);
        }
        // constants of the pruning bound (cell_bound in tls_kernels.hip.h), rounded outwards
        double vq = 0.0;
        for (int64_t j = 0; j < len; ++j) {
            const double dq = (1 - tmpl->values[tmpl->offset[r] + j]) - s1 / (double)len;
            vq += dq * dq;
        }
        we.var_q = vq * (1 + 1e-12);
        we.k_mono = s1 - we.overshoot * s2;
        we.prunable = (len == wd && we.k_mono >= 0 && we.overshoot > 0 && params->transit_depth_min >= 0) ? 1 : 0;
        we.k_mono *= (1 + 1e-12);
        we.c_proxy = 4 * we.overshoot * we.k_mono;
        {   // fp32 screen (tlsdev::screen_cells): |B32 - B| <= screen_c * max|e|, doubled for the statistic's 2 rs B
            const int S = we.tiled ? (tlsdev::kR - 1) * we.xth : 0;
            we.screen_c = 2.0 * (1 + 1e-6) * ((double)(len + S) / 2 + 8) * 5.9604644775390625e-08 * 1.001 * s_abs;
        }
        size_t row_total = front + (size_t)len + 1 + back;   // (+1: the row of difference taps, one tap longer, shares the layout)
        row_total = (row_total + 7) / 8 * 8;
        if (q) q->resize(q_count + row_total, 0.0);
        q_count += row_total;
        we.sum_q2 = s2;
        widths.push_back(we);
    }
    return TLS_OK;
}

// Piecewise-constant images of the template rows for the pruning bound (tlsdev::window_bound).  All rows are the
// same transit shape resampled to their width (transit.py:98-160), so the segment boundaries are chosen ONCE, as
// fractions of the row length, on the widest row: the kSeg-segment partition with the smallest sum of squared
// deviations from the segment means (dynamic programme over <= 96 groups of taps).  Levels, telescoped
// differences and the squared remainder are then exact sums over each row's own taps (long double, remainder
// rounded up): the bound is rigorous for ANY boundaries, good ones only make it tight.
void build_screens(const std::vector<tlsdev::WidthEntry>& widths, const std::vector<double>& q,
                   std::vector<tlsdev::RowScreen>& screens, bool one_segment_only) {
    constexpr int K = tlsdev::kSeg;
    screens.assign(widths.size(), tlsdev::RowScreen());
    for (auto& sc : screens) { std::memset(&sc, 0, sizeof sc); }
    if (widths.empty()) return;
    double frac[K + 1];
    {
        const auto& we = widths.back();
        const int L = we.q_len, G = std::min(L, 96);
        const double* qr = q.data() + we.q_offset;
        std::vector<long double> s1((size_t)G + 1, 0.0L), s2((size_t)G + 1, 0.0L);
        std::vector<int> edge((size_t)G + 1);
        for (int g = 0; g <= G; ++g) edge[(size_t)g] = (int)((long long)g * L / G);
        for (int g = 0; g < G; ++g) {
            long double a1 = 0, a2 = 0;
            for (int j = edge[(size_t)g]; j < edge[(size_t)g + 1]; ++j) { a1 += qr[j]; a2 += (long double)qr[j] * qr[j]; }
            s1[(size_t)g + 1] = s1[(size_t)g] + a1; s2[(size_t)g + 1] = s2[(size_t)g] + a2;
        }
        auto sse = [&](int a, int b) -> double {
            const long double m = (long double)(edge[(size_t)b] - edge[(size_t)a]);
            const long double d1 = s1[(size_t)b] - s1[(size_t)a];
            return (double)((s2[(size_t)b] - s2[(size_t)a]) - d1 * d1 / m);
        };
        const int Ke = std::min(K, G);
        std::vector<double> cost((size_t)(Ke + 1) * (G + 1), 1e300);
        std::vector<int> arg((size_t)(Ke + 1) * (G + 1), 0);
        cost[0] = 0.0;
        for (int k = 1; k <= Ke; ++k)
            for (int j = k; j <= G; ++j) {
                double best = 1e300; int bi = k - 1;
                for (int i = k - 1; i < j; ++i) {
                    const double c = cost[(size_t)(k - 1) * (G + 1) + i] + sse(i, j);
                    if (c < best) { best = c; bi = i; }
                }
                cost[(size_t)k * (G + 1) + j] = best; arg[(size_t)k * (G + 1) + j] = bi;
            }
        int at = G;
        for (int k = K; k >= 0; --k) frac[k] = 1.0;
        for (int k = Ke; k >= 1; --k) { frac[k] = (double)edge[(size_t)at] / L; at = arg[(size_t)k * (G + 1) + at]; }
        frac[0] = 0.0;
        for (int k = Ke + 1; k <= K; ++k) frac[k] = 1.0;
    }
    for (size_t w = 0; w < widths.size(); ++w) {
        const auto& we = widths[w];
        tlsdev::RowScreen& sc = screens[w];
        const int L = we.q_len;
        if (!we.prunable || L < tlsdev::kScreenMinLen || L < 2 * K) continue;
        const double* qr = q.data() + we.q_offset;
        int b[K + 1];
        b[0] = 0;
        for (int k = 1; k < K; ++k) b[k] = std::max(b[k - 1] + 1, (int)std::lround(frac[k] * L));
        b[K] = L;
        for (int k = K - 1; k >= 1; --k) b[k] = std::min(b[k], b[k + 1] - 1);
        long double lev[K], r2 = 0.0L, sq = 0.0L;
        for (int k = 0; k < K; ++k) {
            long double a1 = 0.0L;
            for (int j = b[k]; j < b[k + 1]; ++j) a1 += qr[j];
            lev[k] = a1 / (long double)(b[k + 1] - b[k]);
        }
        // the device works with the levels rounded to double: remainder and sum are those of the ROUNDED levels
        double levd[K];
        for (int k = 0; k < K; ++k) levd[k] = (double)lev[k];
        long double dsum = 0.0L;   // sum of the differences q - q~: zero for exact means, ~1e-17 L after rounding
        for (int k = 0; k < K; ++k)
            for (int j = b[k]; j < b[k + 1]; ++j) {
                const long double dq = (long double)qr[j] - (long double)levd[k];
                r2 += dq * dq; dsum += dq; sq += (long double)levd[k];
            }
        for (int k = 0; k <= K; ++k) sc.b[k] = b[k];
        sc.g[0] = -levd[0];
        for (int k = 1; k < K; ++k) sc.g[k] = levd[k - 1] - levd[k];
        sc.g[K] = levd[K - 1];
        // (g_k is the rounded difference of two doubles: the telescoped sum then equals sum_j q~'_j e_j for levels
        // q~' within 1 ulp of levd -- absorbed by inflating the remainder; |dsum| * mean enters the same way)
        sc.sq = (double)sq;
        sc.r2 = (double)(r2 * (1.0L + 1e-9L)) + 1e-24 + 1e-12 * (double)fabsl(dsum);
        sc.valid = one_segment_only ? 0 : 1;   // developer switch (switch no_screen): the one-segment bound (cell_bound) for every row
    }
}


// scatter of the flux itself: the noise estimate behind pruning_pays (a caller's dy may be in
// arbitrary units -- validate.py:18 normalises it by its mean -- so it says nothing about the noise)
double flux_scatter(const double* y, int64_t n) {
    long double m = 0.0L, v = 0.0L;
    for (int64_t i = 0; i < n; ++i) m += y[i];
    m /= (long double)n;
    for (int64_t i = 0; i < n; ++i) v += (y[i] - m) * (y[i] - m);
    return (double)std::sqrt((double)(v / (long double)n));
}

// the search kernel variant of the next launch, from the scatter of its flux (a batch: the mean over the curves of its group)
void choose_flux_kernels(tls_ctx* ctx, double sigma) {
    ctx->flux = choose_flux_kernels(ctx->plan, ctx->opt, ctx->host_widths, sigma, ctx->depth_min,
                                    screen_admissible(ctx->plan.resident, ctx->plan.uniform, ctx->e_abs_max));
}




// words of d_perm: a stashed order per workgroup in flight (n entries of the classic family's index type; a row of the
// four-slot kernel in the plan's layout, tlsdev::slim_perm_row 16-bit entries)
size_t perm_scratch_words(const tls_ctx* ctx, size_t n) {
    size_t per_block = n;
    if (ctx->plan.slim_blocks > 0) per_block = std::max(per_block, (size_t)tlsdev::slim_perm_row(ctx->plan.slim_threads) / 2);
    return (size_t)std::max(ctx->plan.blocks, ctx->plan.slim_blocks) * per_block;
}


// the two-role kernel of the slab path (fold role, then search role over (period, tile) items)
template <bool UNI, bool COUNTING = false>
hipError_t launch_split(tls_ctx* ctx, const tlsdev::SearchArgs& args, int blocks) {
    auto kernel = tlsdev::tls_fold_search_kernel<UNI, COUNTING>;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)ctx->plan.lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3((unsigned)ctx->plan.threads), ctx->plan.lds_bytes,
                       main_stream(ctx), args);
    return hipGetLastError();
}

template <bool RES, bool UNI, typename IdxT, bool PRUNING = false, bool COUNTING = false, bool SCREEN = false>
hipError_t launch_variant(tls_ctx* ctx, const tlsdev::SearchArgs& args, int blocks) {
    auto kernel = tlsdev::tls_search_kernel<RES, UNI, IdxT, PRUNING, COUNTING, SCREEN>;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)ctx->plan.lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3((unsigned)ctx->plan.threads), ctx->plan.lds_bytes,
                       main_stream(ctx), args);
    return hipGetLastError();
}

// the event pair around one search (tls_kernel_timing adds them up): one kernel, or the fold + search kernels of all
// batches of the two-kernel slab path
hipError_t timing_pair(tls_ctx* ctx, std::pair<hipEvent_t, hipEvent_t>** out) {
    if (ctx->ev_pool.size() < kEventRing) {   // a ring: a long-lived survey process never grows it
        hipEvent_t a, b;
        hipError_t e;
        if ((e = hipEventCreate(&a)) != hipSuccess || (e = hipEventCreate(&b)) != hipSuccess) return e;
        ctx->ev_pool.emplace_back(a, b);
    }
    ctx->ev_overlapped.resize(kEventRing, 0);
    ctx->ev_overlapped[ctx->ev_used % kEventRing] = 0;
    *out = &ctx->ev_pool[ctx->ev_used++ % kEventRing];
    return hipSuccess;
}

// lane B's stream, events and buffers, sized for the plan the context holds (first use, or a larger plan since)
int ensure_lane_b(tls_ctx* ctx) {
    auto& lb = ctx->lane_b;
    if (!lb.stream) TLS_HIP(ctx, hipStreamCreateWithFlags(&lb.stream, hipStreamNonBlocking));
    if (!lb.ev_done) TLS_HIP(ctx, hipEventCreateWithFlags(&lb.ev_done, hipEventDisableTiming));
    if (!lb.ev_stage) TLS_HIP(ctx, hipEventCreateWithFlags(&lb.ev_stage, hipEventDisableTiming));
    if (!lb.d_squeue.ptr) {   // zero once: the kernel rewinds its queue itself
        TLS_HIP(ctx, lb.d_squeue.reserve(4));
        TLS_HIP(ctx, hipMemsetAsync(lb.d_squeue.ptr, 0, 4 * sizeof(unsigned int), lb.stream));
    }
    TLS_HIP(ctx, lb.d_lists.reserve(ctx->d_lists.cap));
    TLS_HIP(ctx, lb.d_perm.reserve(ctx->d_perm.cap));
    TLS_HIP(ctx, lb.d_out.reserve(3 * (size_t)ctx->plan.n_periods + 4));
    TLS_HIP(ctx, lb.d_y.reserve((size_t)ctx->plan.n));
    return TLS_OK;
}

// lane B's next command sees lane A's state as of the latest record of ev_state
int lane_b_see_state(tls_ctx* ctx) {
    auto& lb = ctx->lane_b;
    if (!lb.saw_state) {
        TLS_HIP(ctx, hipStreamWaitEvent(lb.stream, ctx->ev_state, 0));
        lb.saw_state = true;
    }
    return TLS_OK;
}

// lane: -1 a launch outside the lane path (lane A's buffers, behind everything: joined); 0 / 1 an overlappable launch on
// lane A / lane B (tls_execute decides)
int enqueue(tls_ctx* ctx, bool count_work, bool phase_clock = false, double* debug_folded = nullptr, double* debug_prefix = nullptr,
            unsigned long long* period_cycles = nullptr, int lane = -1) {
    auto& lb = ctx->lane_b;
    hipStream_t stream = nullptr;
    const bool filled_before = ctx->perm_filled;
    const bool overlapped = lane >= 0 && ctx->run_lane >= 0;   // (the launch before it may still run when this one begins)
    if (lane < 0) {
        stream = main_stream(ctx);
    } else if (lane == 0) {
        stream = ctx->lane_a_stream;
        if (ctx->state_dirty) {   // (covers the plan's uploads, the filling launch and every consumer so far; not this launch)
            TLS_HIP(ctx, hipEventRecord(ctx->ev_state, stream));
            ctx->state_dirty = false; lb.saw_state = false; ctx->a_reads_flux_b = false;
        }
        if (ctx->flux_lane == 1 && ctx->flux_b_unseen) {
            TLS_HIP(ctx, hipStreamWaitEvent(stream, lb.ev_stage, 0));
            ctx->flux_b_unseen = false;
        }
    } else {
        if (int rc = ensure_lane_b(ctx)) return rc;
        if (int rc = lane_b_see_state(ctx)) return rc;
        stream = lb.stream;
    }
    if (ctx->flux_lane == 1 && lane != 1) ctx->a_reads_flux_b = true;
    if (ctx->flux_lane == 0 && lane == 1) ctx->b_reads_flux_a = true;
    point_results(ctx, lane == 1 ? 1 : 0);
    if (count_work)
        TLS_HIP(ctx, hipMemsetAsync(ctx->d_counters.ptr, 0, 3 * sizeof(unsigned long long), stream));
    tlsdev::SearchArgs a;
    a.t = ctx->d_t.ptr; a.y = ctx->over_y ? ctx->over_y : ctx->d_y.ptr;
    a.w = ctx->plan.uniform ? nullptr : (ctx->over_w ? ctx->over_w : ctx->d_w.ptr);
    a.periods = ctx->d_periods.ptr; a.order = ctx->d_order.ptr; a.rows = ctx->d_rows.ptr;
    a.widths = ctx->d_widths.ptr; a.q = ctx->d_q.ptr; a.q2 = ctx->plan.uniform ? nullptr : ctx->d_q2.ptr;
    a.q32 = ctx->plan.uniform ? reinterpret_cast<const float*>(ctx->d_q2.ptr) : nullptr;
    a.g = ((ctx->plan.resident && ctx->plan.slim_blocks == 0) || (!ctx->plan.resident && ctx->opt.x_staged == 2)) ? nullptr : ctx->d_g.ptr;   // (x_staged = 2: A/B switch, X at staging time but the dot products on the re-staged samples)
    a.split_lo = nullptr; a.park_cells = nullptr; a.e_abs_max = ctx->e_abs_max; a.q32_shifted = ctx->q_count;
    a.screens = ctx->d_screens.ptr;
    a.out_chi2 = ctx->over_chi2 ? ctx->over_chi2 : ctx->d_chi2.ptr;
    a.out_row = ctx->over_row ? ctx->over_row : ctx->d_row.ptr;
    a.out_depth = ctx->over_depth ? ctx->over_depth : ctx->d_depth.ptr;
    a.counters = count_work ? ctx->d_counters.ptr : nullptr;
    a.phase_cycles = nullptr;
    if (phase_clock) {
        TLS_HIP(ctx, ctx->d_phase.reserve(tlsdev::kPhases));
        TLS_HIP(ctx, hipMemsetAsync(ctx->d_phase.ptr, 0, tlsdev::kPhases * sizeof(unsigned long long), stream));
        a.phase_cycles = ctx->d_phase.ptr;
    }
    a.debug_folded = debug_folded; a.debug_prefix = debug_prefix; a.period_cycles = period_cycles;
    a.check = nullptr; a.lds_bytes = (long long)ctx->plan.lds_bytes;
#ifdef TLS_DEBUG_CHECKS
    if (int rc = ensure_check_counters(ctx)) return rc;
    a.check = ctx->d_check.ptr;
#endif
    a.queue = lane == 1 ? lb.d_squeue.ptr : ctx->d_squeue.ptr;
    a.claim_ahead = 0;
    a.scratch = ctx->d_scratch.ptr;
    a.scratch_stride = (long long)(ctx->plan.uniform ? 2 : 3) * ((ctx->plan.M + 1 + ctx->plan.region_pad + 1) & ~1);   // even regions (kernel: RS)
    a.region_pad = ctx->plan.region_pad;
    a.chunk_lists = lane == 1 ? lb.d_lists.ptr : ctx->d_lists.ptr; a.list_stride = 3 * (long long)ctx->plan.list_stride; a.list_cap = (long long)ctx->plan.list_stride;
    a.prune_min_live = ctx->plan.prune_min_live; a.p2_shift = ctx->plan.p2_shift; a.hdr_bytes = ctx->plan.hdr_bytes; a.tile_len = ctx->plan.tile_len; a.tile_halo = ctx->plan.tile_halo;
    a.depth_min = ctx->depth_min; a.S0 = ctx->S0; a.w0 = ctx->w0;
    a.cumsum_round = ctx->plan.cumsum_round;
    {
        // the sequential cumsum C of the reference (helpers.py:72) rounds by at most half an ulp of its running value
        // per step, and C <= (n + W) * max|flux|: the two constants below follow from that (tls_kernels.hip.h,
        // depth_pass and window_bound)
        const double c_max = (double)ctx->plan.M * ctx->y_abs_max;
        // (band half-width: 1.25 x the bound 2^-53 c_max on |dX/d - mean_reference|, plus 1e-14 for what the bound leaves out --
        // the plain scan's own rounding, <= ~20 * 2^-53 * max|X| / d, and the reference's division; rounds 3 and early 4
        // shipped 2 x: twice the second attempts for no additional safety)
        a.eps_fast = fast_mode_eps(ctx->plan.M, ctx->y_abs_max);
        a.slack_unit = 2.5e-16 * c_max;
        a.exact_prefix = ctx->opt.exact_prefix == 1 ? 1 : 0;
        // Series in the HBM slab, one-workgroup-per-period kernel: fast mode too (switch fast_slab = 0: exact mode).
        // The band grows with the series (eps ~ 2^-52 (n + W) max|flux|) while the noise of a window mean shrinks: 2.6 % of
        // the TESS-size and 10 % of the Kepler-size periods hit it and go through the prefix sum and phase 3 a second time
        // (the folded flux is kept).  Round 4, same box: Kepler full grid 275.8 -> 254.8 ms, TESS 2.97 -> 2.90 ms.
        // WHICH mode a period takes depends on the light curve and the period alone (the expectation below) -- never on how
        // many other periods the launch holds or on the device: a shard of a multi-GPU search returns the bits of the
        // full-grid search.  (Round 4 kept launches of <= 4 rounds exact to spare them a late second attempt; a period's
        // bits then depended on the launch.  The queue order now sends the periods most likely to need one first.)
        a.fast_slab = ctx->opt.fast_slab == 0 ? 0 : 1;
    }
    a.x_at_staging = 0;
    if (!ctx->plan.resident && a.fast_slab) {
        a.x_at_staging = ctx->plan.any_oversize ? 0 : 1;   // (rows evaluated straight from the slab list their cells with the first tile: they need all of X)
        if (ctx->opt.x_staged == 0) a.x_at_staging = 0;
    }
    a.band_prefix = nullptr;
    a.band_max = ctx->opt.band_max >= 0 ? ctx->opt.band_max : kBandMax;
    if (!ctx->plan.resident && a.fast_slab && ctx->flux.sigma > 0 &&
        !(ctx->band_sigma == ctx->flux.sigma && ctx->band_eps == a.eps_fast && ctx->d_band_now)) {
        // the band expectation of every width row (band_prefix_for), as a prefix over the width table: the kernel forms a
        // period's expectation from its duration window [k_lo, k_hi).  Uploaded from one of two pinned slots, nothing is
        // waited for (a survey changes sigma with every group of light curves: the launch in flight keeps reading its own slot).
        const size_t cnt = ctx->host_widths.size() + 1;
        if (ctx->h_band_cap < 2 * cnt) {
            TLS_HIP(ctx, hipStreamSynchronize(stream));
            if (ctx->h_band) TLS_HIP(ctx, hipHostFree(ctx->h_band));
            ctx->h_band = nullptr; ctx->h_band_cap = 0;
            TLS_HIP(ctx, hipHostMalloc(reinterpret_cast<void**>(&ctx->h_band), 2 * cnt * sizeof(double), hipHostMallocDefault));
            ctx->h_band_cap = 2 * cnt;
            TLS_HIP(ctx, ctx->d_band.reserve(2 * cnt));
            for (auto& ev : ctx->ev_band) if (!ev) TLS_HIP(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            ctx->band_used[0] = ctx->band_used[1] = false;
        }
        const int slot = ctx->band_slot ^= 1;
        if (ctx->band_used[slot]) TLS_HIP(ctx, hipEventSynchronize(ctx->ev_band[slot]));   // (two uploads ago: long done)
        double* h = ctx->h_band + (size_t)slot * cnt;
        std::vector<double> pre;
        band_prefix_for(ctx->host_widths, ctx->flux.sigma, ctx->depth_min, a.eps_fast, pre);
        std::memcpy(h, pre.data(), cnt * sizeof(double));
        ctx->d_band_now = ctx->d_band.ptr + (size_t)slot * cnt;
        TLS_HIP(ctx, hipMemcpyAsync(ctx->d_band_now, h, cnt * sizeof(double), hipMemcpyHostToDevice, stream));
        TLS_HIP(ctx, hipEventRecord(ctx->ev_band[slot], stream));
        ctx->band_used[slot] = true;
        ctx->band_sigma = ctx->flux.sigma; ctx->band_eps = a.eps_fast;
    }
    if (!ctx->plan.resident && a.fast_slab && ctx->flux.sigma > 0) a.band_prefix = ctx->d_band_now;
    a.sort2 = ctx->plan.sort2 ? 1 : 0;
    a.n_curves = ctx->batch_curves;
    a.curve_S0 = ctx->over_S0 ? ctx->over_S0 : ctx->d_curve_S0.ptr;
    a.curve_w0 = ctx->over_w0 ? ctx->over_w0 : ctx->d_curve_w0.ptr;
    a.perm_scratch = lane == 1 ? lb.d_perm.ptr : ctx->d_perm.ptr;
    a.perm_table = nullptr; a.perm_filled = 0; a.perm_per = 0;
    a.n = ctx->plan.n; a.W = ctx->plan.W; a.M = ctx->plan.M;
    a.n_periods = ctx->plan.n_periods; a.n_widths = ctx->plan.n_widths; a.nb = ctx->plan.nb;
    a.batch_lo = 0; a.batch_n = 0; a.tile_prefix = ctx->d_tile_prefix.ptr;
    a.partials = ctx->d_partials.ptr; a.tiles_done = ctx->d_tiles_done.ptr;
    a.fold_ready = ctx->d_tiles_done.ptr ? ctx->d_tiles_done.ptr + ctx->plan.split_batch : nullptr;   // (only the two-role plan has them)
    a.split_fast = ctx->plan.split_fast && a.x_at_staging && a.g != nullptr ? 1 : 0;
    hipError_t e;
    std::pair<hipEvent_t, hipEvent_t>* evp = nullptr;
    if ((e = timing_pair(ctx, &evp)) != hipSuccess) return fail(ctx, TLS_E_HIP, std::string("timing events: ") + hipGetErrorString(e));
    if ((e = hipEventRecord(evp->first, stream)) != hipSuccess) {
        --ctx->ev_used;
        return fail(ctx, TLS_E_HIP, std::string("timing events: ") + hipGetErrorString(e));
    }
    const SearchPlan& plan = ctx->plan;
    const Kernel kernel_pick = pick_kernel(plan, ctx->flux, LaunchFlags{count_work, debug_folded || debug_prefix, ctx->batch_curves});
    if (lane >= 0 && !is_slim(kernel_pick)) { --ctx->ev_used; return fail(ctx, TLS_E_STATE, "launch lanes: not a four-slot launch"); }
    // (counting has an instantiation of its own: the plain kernels do not keep the counters)
    switch (kernel_pick) {
    case Kernel::ResidentScreen: {
        const size_t region = (size_t)plan.M + 1 + (size_t)plan.region_pad;
        hipError_t er = static_cast<hipError_t>(ctx->d_split.reserve((size_t)plan.blocks * region));
        if (er != hipSuccess) { --ctx->ev_used; return fail(ctx, TLS_E_HIP, std::string("fp32 screen scratch: ") + hipGetErrorString(er)); }
        a.split_lo = ctx->d_split.ptr;
        er = static_cast<hipError_t>(ctx->d_park.reserve((size_t)plan.blocks * tlsdev::kParkCap * 2));   // (a ParkedCell is two doubles wide)
        if (er != hipSuccess) { --ctx->ev_used; return fail(ctx, TLS_E_HIP, std::string("fp32 screen scratch: ") + hipGetErrorString(er)); }
        a.park_cells = ctx->d_park.ptr;
        e = launch_variant<true, true, unsigned short, false, false, true>(ctx, a, plan.blocks);
        break;
    }
    case Kernel::Slim:
    case Kernel::Slim512: {
        a.lds_bytes = (long long)plan.slim_lds;
        a.perm_table = ctx->perm_table_entries ? ctx->d_perm_table.ptr : nullptr; a.perm_filled = ctx->perm_filled ? 1 : 0;
        a.perm_per = plan.slim_perm_per;
        a.claim_ahead = claim_ahead_bits(ctx->opt);
        // (switch dense_hoist = 0: the instantiations whose fast-mode dense predicate is the loop exact mode keeps)
        auto kernel = ctx->opt.dense_hoist != 0
                          ? (kernel_pick == Kernel::Slim512
                                 ? (count_work ? tlsdev::tls_slim_kernel<true, tlsdev::kSlimThreadsWide> : tlsdev::tls_slim_kernel<false, tlsdev::kSlimThreadsWide>)
                                 : (count_work ? tlsdev::tls_slim_kernel<true, tlsdev::kSlimThreads> : tlsdev::tls_slim_kernel<false, tlsdev::kSlimThreads>))
                          : (kernel_pick == Kernel::Slim512
                                 ? (count_work ? tlsdev::tls_slim_kernel<true, tlsdev::kSlimThreadsWide, false> : tlsdev::tls_slim_kernel<false, tlsdev::kSlimThreadsWide, false>)
                                 : (count_work ? tlsdev::tls_slim_kernel<true, tlsdev::kSlimThreads, false> : tlsdev::tls_slim_kernel<false, tlsdev::kSlimThreads, false>));
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.slim_lds);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)plan.slim_blocks), dim3((unsigned)plan.slim_threads), plan.slim_lds, stream, a);
            e = hipGetLastError();
        }
        if (e == hipSuccess && a.perm_table) ctx->perm_filled = true;   // (every period of the plan passes through a launch)
        break;
    }
    case Kernel::Resident:
    case Kernel::ResidentPrune:
        e = !plan.uniform ? (count_work ? launch_variant<true, false, unsigned short, false, true>(ctx, a, plan.blocks)
                                        : launch_variant<true, false, unsigned short, false, false>(ctx, a, plan.blocks))
            : kernel_pick == Kernel::ResidentPrune ? launch_variant<true, true, unsigned short, true, false>(ctx, a, plan.blocks)
            : count_work  ? launch_variant<true, true, unsigned short, false, true>(ctx, a, plan.blocks)
                          : launch_variant<true, true, unsigned short, false, false>(ctx, a, plan.blocks);
        break;
    case Kernel::Slab:
        e = !plan.uniform ? (count_work ? launch_variant<false, false, unsigned int, false, true>(ctx, a, plan.blocks)
                                        : launch_variant<false, false, unsigned int, false, false>(ctx, a, plan.blocks))
            : count_work  ? launch_variant<false, true, unsigned int, false, true>(ctx, a, plan.blocks)
                          : launch_variant<false, true, unsigned int, false, false>(ctx, a, plan.blocks);
        break;
    case Kernel::SlabSplit:
        // series in the HBM slab, one light curve: per batch of periods ONE launch of the two-role kernel -- every
        // workgroup folds periods of the batch until none is left (one slab per period), then searches (period, tile) items
        e = hipSuccess;
        for (int lo = 0; lo < plan.n_periods && e == hipSuccess; lo += plan.split_batch) {
            a.batch_lo = lo; a.batch_n = std::min(plan.split_batch, plan.n_periods - lo);
            a.queue = ctx->d_squeue.ptr;   // [0..1] the fold role's queue, [2..3] the search role's
            const int64_t items = (int64_t)plan.tile_prefix[(size_t)(lo + a.batch_n)] - (int64_t)plan.tile_prefix[(size_t)lo];
            const int blocks = (int)std::min<int64_t>(plan.split_blocks, std::max<int64_t>(items, 1));
            e = !plan.uniform ? (count_work ? launch_split<false, true>(ctx, a, blocks) : launch_split<false, false>(ctx, a, blocks))
                : count_work  ? launch_split<true, true>(ctx, a, blocks)
                              : launch_split<true, false>(ctx, a, blocks);
        }
        break;
    }
    // (a failure from here on gives the event pair back: tls_kernel_timing must not meet a pair whose second event was
    // never recorded)
    if (e != hipSuccess) { --ctx->ev_used; return fail(ctx, TLS_E_HIP, std::string("kernel launch: ") + hipGetErrorString(e)); }
    if ((e = hipEventRecord(evp->second, stream)) != hipSuccess) {
        --ctx->ev_used;
        return fail(ctx, TLS_E_HIP, std::string("timing events: ") + hipGetErrorString(e));
    }
    ctx->ev_overlapped[(ctx->ev_used - 1) % kEventRing] = overlapped ? 1 : 0;
    if (lane == 1) {
        TLS_HIP(ctx, hipEventRecord(lb.ev_done, stream));
        lb.outstanding = true;
    }
    ctx->perm_filled_before_prev = filled_before;
    ctx->run_lane = lane;   // (-1: the launch ends a run of overlappable ones)
    ++ctx->lane_launches[lane == 1 ? 1 : 0];
    ctx->executed = true;
    ctx->counted = count_work;
    ctx->last_kernel = kernel_name(kernel_pick);
    return TLS_OK;
}

// tls_t0fit_kernel's layout (tls_transit_models shares it): a 272-byte header, then 16 bytes a point where the series fits
// the LDS and its order 16 bits; else up to 16384 sort buckets, the series in HBM scratch
struct T0FitShape { bool resident; int nb; size_t lds; };
T0FitShape t0fit_shape(int64_t n) {
    const size_t hdr = 272, resident_bytes = hdr + 16 * (size_t)n;
    T0FitShape s;
    s.resident = resident_bytes <= kLdsPerCU && n <= 65535;
    s.nb = s.resident ? (int)n : (int)std::min<int64_t>(n, 16384);
    s.lds = s.resident ? resident_bytes : hdr + 4 * (size_t)s.nb;
    return s;
}

// T0-fit launch shared by tls_t0_fit and tls_power_batch: every pointer on the device, nothing waited for.
// One fit (d_params == nullptr: period, dur, roll, n_epochs from the host) or `n_fits` fits in ONE launch (their parameters,
// epochs and signals written on the device by tls_power_prep, the arrays `*_stride` doubles apart).
// Three launches (round 6): the base order of every fit (one workgroup a fit), the epochs as rotations of it (one wavefront
// an epoch: tls_t0fit_rot), and the general kernel for the fits the rotation path handed back (ties, gaps the folds' rounding
// could close: its workgroups pass over the other fits).  Switch t0_rot = 0: the general kernel alone.  The general kernel's
// `blocks` workgroups go through the fits one after the other: HBM scratch (series that do not fit the LDS) is one slab per
// workgroup, max(blocks, n_fits) slabs in all (mode 1 has one workgroup per fit), whatever the number of fits.
// d_curve: nullptr, or the curve of every fit (T0FitArgs::curve: several fits read one light curve's flux).
int launch_t0_fit(tls_ctx* ctx, const double* d_t, const double* d_y, const double* d_signal, const double* d_epochs,
                  double* d_residuals, unsigned int* d_queue, int64_t n, double period, int64_t dur, int64_t n_epochs,
                  int64_t roll, double t_lo, double t_hi, const tlsdev::T0FitParams* d_params = nullptr, int64_t n_fits = 1,
                  int64_t y_stride = 0, int64_t signal_stride = 0, int64_t epoch_stride = 0, const int* d_curve = nullptr) {
    tlsdev::T0FitArgs a;
    a.t = d_t; a.y = d_y; a.signal = d_signal; a.epochs = d_epochs;
    a.residuals = d_residuals; a.queue = d_queue; a.scratch = nullptr; a.scratch_stride = 0;
    a.period = period; a.n = (int)n; a.dur = (int)dur; a.roll = (int)(roll % n); a.n_epochs = (int)n_epochs;
    a.params = d_params; a.y_stride = y_stride; a.signal_stride = signal_stride; a.epoch_stride = epoch_stride;
    a.curve = d_curve;
    a.n_fits = d_params ? (int)n_fits : 1;
    a.mode = 0; a.rot = nullptr; a.rot_perm = nullptr; a.rot_stride = 0; a.t_lo = t_lo; a.t_hi = t_hi;
    const T0FitShape shape = t0fit_shape(n);
    const bool resident = shape.resident;
    const size_t lds = shape.lds;
    a.nb = shape.nb;
    int threads, blocks;
    // (a batched launch does not know its fits' epoch counts on the host: every fit gets the full set of workgroups, those
    // beyond its epochs pass it over)
    const int64_t epochs_cap = d_params ? n : n_epochs;
    if (resident) {
        const size_t per_cu = kLdsPerCU / lds;
        threads = per_cu >= 2 ? 512 : 1024;
        const size_t wg_per_cu = std::min<size_t>(per_cu, 2048 / (size_t)threads);
        blocks = (int)std::min<int64_t>(epochs_cap, (int64_t)wg_per_cu * ctx->n_cu);
    } else {
        threads = 512; blocks = (int)std::min<int64_t>(epochs_cap, (int64_t)2 * ctx->n_cu);
        a.scratch_stride = 3 * n;
        TLS_HIP(ctx, ctx->d_fscratch.reserve((size_t)std::max<int64_t>(blocks, n_fits) * (size_t)a.scratch_stride));
        a.scratch = ctx->d_fscratch.ptr;
    }
    if (blocks < 1) return TLS_OK;
    const unsigned fits = (unsigned)std::max<int64_t>(n_fits, 1);
    const bool rotation = ctx->opt.t0_rot != 0 && n >= tlsdev::kT0RotMinPoints;
    if (rotation) {
        a.rot_stride = 3 * (long long)n + 4;
        TLS_HIP(ctx, ctx->d_frot.reserve((size_t)fits * (size_t)a.rot_stride));
        TLS_HIP(ctx, ctx->d_frperm.reserve((size_t)fits * (size_t)n));
        a.rot = ctx->d_frot.ptr; a.rot_perm = ctx->d_frperm.ptr;
    }
    auto launch = [&](int mode, unsigned grid_x) -> hipError_t {
        tlsdev::T0FitArgs b = a;
        b.mode = mode;
        const dim3 grid(grid_x, mode == 1 ? fits : 1u);
        hipError_t e;
        if (resident) {
            auto kernel = tlsdev::tls_t0fit_kernel<true, unsigned short>;
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e == hipSuccess) { hipLaunchKernelGGL(kernel, grid, dim3((unsigned)threads), lds, main_stream(ctx), b); e = hipGetLastError(); }
        } else {
            auto kernel = tlsdev::tls_t0fit_kernel<false, unsigned int>;
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e == hipSuccess) { hipLaunchKernelGGL(kernel, grid, dim3((unsigned)threads), lds, main_stream(ctx), b); e = hipGetLastError(); }
        }
        return e;
    };
    hipError_t e = hipSuccess;
    if (rotation) {
        e = launch(1, 1u);
        if (e == hipSuccess) {
            const unsigned waves_per_wg = 4;
            const dim3 grid((unsigned)((epochs_cap + waves_per_wg - 1) / waves_per_wg), fits);
            hipLaunchKernelGGL(tlsdev::tls_t0fit_rot, grid, dim3(waves_per_wg * 64), 0, main_stream(ctx), a);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = launch(2, (unsigned)blocks);
    } else {
        e = launch(0, (unsigned)blocks);
    }
    if (e != hipSuccess) return fail(ctx, TLS_E_HIP, std::string("t0 fit launch: ") + hipGetErrorString(e));
    return TLS_OK;
}

// ---- the post-search chain of survey-mode power() (tls_power_batch; tls_debug_post_search feeds it injected search results):
// spectra (stats.py:105-132), the pick of main.py:198-212,269-272, trial epochs and scaled template (tls_power_prep), the
// final T0 fit of every curve in one set of launches (stats.py:135-204) and its first minimum, nothing waited for
struct PostSearchBufs {
    size_t spec_stride = 0, fit_stride = 0;   // SR | power_raw | power of one curve; epochs / residuals of one fit
    int64_t max_len = 1;                       // longest template row: the stride of the scaled signals
    double *sde = nullptr, *pick = nullptr, *T0 = nullptr;   // [group][2] | [group][8] | [group], side by side (ONE copy out)
    double* stats = nullptr;                   // tls_power_batch_stats: [group][16] | per-transit [group][6][max_epochs], behind T0
    double* per_transit = nullptr;             // ... the per-transit rows: behind the records, or behind the peaks where they are not copied out
    double* peaks = nullptr;                   // tls_power_batch_peaks: [group][1 + 6 k], behind what of the statistics is copied out
    double* fits = nullptr;                    // tls_power_batch_peak_fits: T0 [group k] | status [group k] | records [group k][16], behind the peaks
    double* scans = nullptr;                   // tls_power_batch_phase_scan: records [group k][12], behind the peak fits
    int64_t group = 0;
    int* n_epochs = nullptr;
    tlsdev::T0FitParams* fit = nullptr;
};

// stats_words: doubles of the statistics stage per curve behind T0 (0: no statistics requested); peaks_words: of the peaks
// behind the first stats_copied (<= stats_words: the records alone, or the per-transit rows too) of those -- sde | pick | T0 |
// statistics copied out | peaks | peak fits (fits_words doubles a curve, with peaks only) | phase scans (scans_words, with
// peak fits only) are ONE contiguous copy, per-transit rows nobody asked for stay behind it
int reserve_post_search(tls_ctx* ctx, int64_t group, int64_t n_periods, int64_t n, int64_t max_len, PostSearchBufs& b,
                        size_t stats_words = 0, size_t peaks_words = 0, size_t stats_copied = 0, size_t fits_words = 0,
                        size_t scans_words = 0) {
    const size_t np = (size_t)n_periods, g = (size_t)group;
    b.max_len = std::max<int64_t>(max_len, 1);
    b.spec_stride = 3 * np;
    b.group = group;
    // the per-transit rows follow the records where they are copied out with them (or where there are no peaks); else they
    // stay behind everything that is copied
    const size_t record_words = stats_words ? (size_t)tlsdev::kTransitStats : 0, row_words = stats_words - record_words;
    const bool rows_last = peaks_words && stats_copied != stats_words;
    double* spectra;   // (enqueue_post_search reads them from d_spec's start)
    Arena L;
    L.add(spectra, g * b.spec_stride);  L.add(b.sde, 2 * g);  L.add(b.pick, 8 * g);  L.add(b.T0, g);
    L.add(b.stats, record_words * g);
    if (!rows_last) L.add(b.per_transit, row_words * g);
    L.add(b.peaks, peaks_words * g);  L.add(b.fits, fits_words * g);  L.add(b.scans, scans_words * g);
    if (rows_last) L.add(b.per_transit, row_words * g);
    TLS_HIP(ctx, L.bind(ctx->d_spec));
    b.fit_stride = (size_t)n;
    TLS_HIP(ctx, ctx->d_fep.reserve(g * b.fit_stride));
    TLS_HIP(ctx, ctx->d_fres.reserve(g * b.fit_stride));
    double* signals;   // (read from d_fsig's start)
    Arena F;
    F.add(signals, g * (size_t)b.max_len);  F.add(b.n_epochs, 2 * g);   // (a double's room a curve)
    F.add(b.fit, g);
    TLS_HIP(ctx, F.bind(ctx->d_fsig));
    return TLS_OK;
}

// `gc` curves: chi2 / row / depth [gc][n_periods], flux [gc][n] on the device; the plan's time stamps, periods and template
int enqueue_post_search(tls_ctx* ctx, const PostSearchBufs& b, int64_t gc, const double* d_chi2, const long long* d_row,
                        const double* d_depth, const double* d_y, int64_t n, int64_t n_periods, int64_t median_kernel,
                        double t_min, double t_max, double margin) {
    const size_t np = (size_t)n_periods;
    int64_t kernel = median_kernel;
    if (kernel % 2 == 0) kernel += 1;                                   // stats.py:115-117
    tlsdev::SpectraArgs sa;
    sa.chi2 = d_chi2; sa.SR = ctx->d_spec.ptr; sa.power_raw = ctx->d_spec.ptr + np; sa.power = ctx->d_spec.ptr + 2 * np;
    sa.sde = b.sde; sa.n = (int)n_periods; sa.kernel = (int)kernel; sa.detrend = n_periods > 2 * kernel ? 1 : 0;   // stats.py:118
    sa.chi2_stride = (long long)np; sa.out_stride = (long long)b.spec_stride; sa.sde_stride = 2;
    hipLaunchKernelGGL(tlsdev::tls_spectra_head, dim3(1, (unsigned)gc), dim3(1024), 0, main_stream(ctx), sa);
    if (sa.detrend) {
        const int n_med = (int)(n_periods - kernel + 1), per = tlsdev::kMedianWindows;
        const size_t lds = (size_t)(2 * per + kernel) * 8;
        hipLaunchKernelGGL(tlsdev::tls_spectra_median, dim3((unsigned)((n_med + per - 1) / per), (unsigned)gc), dim3(256), lds,
                           main_stream(ctx), sa);
        hipLaunchKernelGGL(tlsdev::tls_spectra_tail, dim3(1, (unsigned)gc), dim3(1024), 0, main_stream(ctx), sa);
    }
    tlsdev::PickArgs pa;
    pa.chi2 = d_chi2; pa.row = d_row; pa.depth = d_depth; pa.power = ctx->d_spec.ptr + 2 * np;
    pa.periods = ctx->d_periods.ptr; pa.out = b.pick; pa.power_stride = (long long)b.spec_stride; pa.n = (int)n_periods;
    hipLaunchKernelGGL(tlsdev::tls_power_pick, dim3((unsigned)gc), dim3(1024), 0, main_stream(ctx), pa);
    // (WITHOUT a host round trip, round 6: trial epochs, the depth-scaled template and the fit's parameters are formed on the
    // device from the pick, all fits run in ONE set of launches, the first minimum is taken on the device)
    tlsdev::PrepArgs pr;
    pr.pick = b.pick; pr.widths = ctx->d_widths.ptr; pr.n_widths = ctx->plan.n_widths; pr.q = ctx->d_q.ptr;
    pr.signal = ctx->d_fsig.ptr; pr.signal_stride = (long long)b.max_len; pr.epochs = ctx->d_fep.ptr; pr.epoch_stride = (long long)b.fit_stride;
    pr.params = b.fit; pr.n_epochs = b.n_epochs; pr.t_min = t_min; pr.margin = margin; pr.n = (int)n;
    hipLaunchKernelGGL(tlsdev::tls_power_prep, dim3((unsigned)gc), dim3(256), 0, main_stream(ctx), pr);
    TLS_HIP(ctx, hipGetLastError());
    int rc = launch_t0_fit(ctx, ctx->d_t.ptr, d_y, ctx->d_fsig.ptr, ctx->d_fep.ptr, ctx->d_fres.ptr, nullptr, n, 1.0, 0, 0, 0,
                           t_min, t_max, b.fit, gc, n, b.max_len, (int64_t)b.fit_stride);
    if (rc) return rc;
    tlsdev::FirstMinArgs fa;
    fa.residuals = ctx->d_fres.ptr; fa.epochs = ctx->d_fep.ptr; fa.n_epochs = b.n_epochs;
    fa.T0 = b.T0; fa.stride = (long long)b.fit_stride;
    hipLaunchKernelGGL(tlsdev::tls_first_min, dim3((unsigned)gc), dim3(1024), 0, main_stream(ctx), fa);
    TLS_HIP(ctx, hipGetLastError());
    return TLS_OK;
}

// ---- the per-transit statistics stage (tls_power_batch_stats; tls_debug_transit_stats feeds it injected picks)
struct StatsRequest {
    const double* row_duration = nullptr; int64_t n_rows = 0;   // lc_cache_overview["duration"] of every template row
    double fill_factor = 0;
    // float(k) ** 0.5 (snr, pink-noise width, depth_mean_std) and numpy.sum(k) ** 0.5 (the odd and even depth errors),
    // k < n_root (n_root > n), each as the caller's Python and numpy form it
    const double* root = nullptr; const double* root_count = nullptr; int64_t n_root = 0;
    int64_t max_epochs = 1;
    tls_transit_stats* out = nullptr; double* out_per_transit = nullptr; int64_t* out_n_epochs = nullptr;
    size_t words() const { return (size_t)tlsdev::kTransitStats + (size_t)tlsdev::kPerTransitRows * (size_t)max_epochs; }
};
static_assert(sizeof(tls_transit_stats) == tlsdev::kTransitStats * 8, "tls_transit_stats is the kernel's record");

struct StatsBufs { double *row_duration = nullptr, *root = nullptr, *root_count = nullptr, *scratch = nullptr; int* ranges = nullptr; size_t scratch_stride = 0; };

// device inputs of a request (uploaded once per call) and the O(group x n) scratch of one group
int reserve_transit_stats(tls_ctx* ctx, const StatsRequest& sr, int64_t group, int64_t n, StatsBufs& sb) {
    sb.scratch_stride = 4 * (size_t)n + 1;   // flux_ootr | concat(odd, even) | pink terms | running sums
    Arena L;
    L.add(sb.row_duration, (size_t)sr.n_rows);  L.add(sb.root, (size_t)sr.n_root);  L.add(sb.root_count, (size_t)sr.n_root);
    L.add(sb.scratch, (size_t)group * sb.scratch_stride);
    TLS_HIP(ctx, L.bind(ctx->d_tstats));
    TLS_HIP(ctx, ctx->d_tranges.reserve((size_t)group * 3 * (size_t)sr.max_epochs));
    sb.ranges = ctx->d_tranges.ptr;
    TLS_HIP(ctx, hipMemcpyAsync(sb.row_duration, sr.row_duration, (size_t)sr.n_rows * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(sb.root, sr.root, (size_t)sr.n_root * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(sb.root_count, sr.root_count, (size_t)sr.n_root * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    return TLS_OK;
}

// the statistics of `gc` curves from the chain's pick, T0 and detrended power (enqueue_post_search), nothing waited for
int enqueue_transit_stats(tls_ctx* ctx, const PostSearchBufs& b, const StatsBufs& sb, const StatsRequest& sr, int64_t gc,
                          const double* d_y, int64_t n, int64_t n_periods, double t_min, double t_max) {
    tlsdev::TransitStatsArgs a;
    a.t = ctx->d_t.ptr; a.y = d_y; a.pick = b.pick; a.T0 = b.T0;
    a.power = ctx->d_spec.ptr + 2 * (size_t)n_periods; a.power_stride = (long long)b.spec_stride;
    a.curve = nullptr;
    a.periods = ctx->d_periods.ptr; a.n_periods = (int)n_periods;
    a.row_duration = sb.row_duration; a.root = sb.root; a.root_count = sb.root_count; a.n_root = (int)sr.n_root;
    a.fill_factor = sr.fill_factor; a.t_min = t_min; a.t_max = t_max;
    a.stats = b.stats; a.per_transit = b.per_transit;
    a.ranges = sb.ranges; a.scratch = sb.scratch; a.scratch_stride = (long long)sb.scratch_stride;
    a.n = (int)n; a.max_epochs = (int)sr.max_epochs;
    hipLaunchKernelGGL(tlsdev::tls_transit_stats, dim3((unsigned)gc), dim3(256), 0, main_stream(ctx), a);
    TLS_HIP(ctx, hipGetLastError());
    return TLS_OK;
}

// curve c's statistics from the group's host copy (records of `group` curves, then their per-transit rows when copied)
int read_transit_stats(tls_ctx* ctx, const StatsRequest& sr, const double* h_stats, int64_t group, int64_t c, int64_t curve,
                       bool with_rows) {
    const double* rec = h_stats + (size_t)tlsdev::kTransitStats * c;
    const double epochs = rec[10];
    if (epochs > (double)sr.max_epochs)
        return fail(ctx, TLS_E_ARG, "light curve " + std::to_string((long long)curve) + " has more than max_epochs = " +
                                    std::to_string((long long)sr.max_epochs) + " transit epochs");
    std::memcpy(&sr.out[curve], rec, sizeof(tls_transit_stats));
    if (sr.out_n_epochs) sr.out_n_epochs[curve] = std::isnan(epochs) ? 0 : (int64_t)epochs;
    if (sr.out_per_transit && with_rows) {
        const size_t rows = (size_t)tlsdev::kPerTransitRows * (size_t)sr.max_epochs;
        std::memcpy(sr.out_per_transit + (size_t)curve * rows, h_stats + (size_t)tlsdev::kTransitStats * group + (size_t)c * rows, rows * 8);
    }
    return TLS_OK;
}

// what the statistics stage requires beyond tls_power_batch's arguments
// (need_out false: the inputs alone, for the peak fits of a call that asks for no statistics of the best pick)
int check_stats_request(tls_ctx* ctx, const StatsRequest& sr, const double* t, int64_t n, int64_t n_rows, bool need_out = true) {
    if (!sr.row_duration || !sr.root || !sr.root_count || (need_out && !sr.out)) return fail(ctx, TLS_E_ARG, "null statistics argument");
    if (sr.n_rows != n_rows) return fail(ctx, TLS_E_ARG, "one fractional duration per template row wanted");
    if (sr.n_root < n + 1) return fail(ctx, TLS_E_ARG, "the two k ** 0.5 tables must cover k = 0 .. n");
    if (sr.max_epochs < 1 || sr.max_epochs > 100000000) return fail(ctx, TLS_E_ARG, "max_epochs out of range [1, 1e8]");
    if (n > 0x3fffffff) return fail(ctx, TLS_E_ARG, "n too large for the statistics stage");
    for (int64_t i = 1; i < n; ++i)
        if (!(t[i] >= t[i - 1])) return fail(ctx, TLS_E_ARG, "the statistics need non-decreasing time stamps");
    return TLS_OK;
}

// ---- the plotted arrays of power() (tls_power_batch_models; tls_debug_transit_models feeds it injected picks): behind the
// statistics stage, whose transit times and epoch counts it reads
struct ModelsRequest {
    const double* curve_t = nullptr; const double* curve_f = nullptr; int64_t curve_n = 0;   // in-transit supersampled curve
    double curve_lo = 0, curve_hi = 0, maxw = 0;
    int64_t lc_cap = 0;                                          // entries of a model light curve row
    double* out_folded = nullptr; double* out_model_folded = nullptr; double* out_lc = nullptr; int64_t* out_lc_len = nullptr;
    size_t stride(int64_t n) const { return (size_t)tlsdev::kModelsHeader + 4 * (size_t)n + 2 * (size_t)lc_cap; }
};
// the two requests from the flat arguments of the C entry points
StatsRequest stats_request(const double* row_duration, int64_t n_rows, double fill_factor, const double* root,
                           const double* root_count, int64_t n_root,
                           int64_t max_epochs, tls_transit_stats* out, double* out_per_transit, int64_t* out_n_epochs) {
    return StatsRequest{row_duration, n_rows, fill_factor, root, root_count, n_root, max_epochs, out, out_per_transit,
                        out_n_epochs};
}
ModelsRequest models_request(const double* curve_t, const double* curve_f, int64_t curve_n, double curve_lo, double curve_hi,
                             double maxw, int64_t lc_cap, double* out_folded, double* out_model_folded, double* out_lc,
                             int64_t* out_lc_len) {
    return ModelsRequest{curve_t, curve_f, curve_n, curve_lo, curve_hi, maxw, lc_cap, out_folded, out_model_folded, out_lc, out_lc_len};
}

struct ModelsBufs { double *curve = nullptr, *scratch = nullptr, *out = nullptr; size_t scratch_stride = 0, out_stride = 0; bool resident = false; int nb = 0; size_t lds = 0; };

int check_models_request(tls_ctx* ctx, const ModelsRequest& mr, int64_t n) {
    if (!mr.curve_t || !mr.curve_f || !mr.out_folded || !mr.out_model_folded || !mr.out_lc || !mr.out_lc_len)
        return fail(ctx, TLS_E_ARG, "null model argument");
    if (mr.curve_n < 2 || mr.curve_n > 100000000) return fail(ctx, TLS_E_ARG, "the template curve needs at least two samples");
    for (int64_t i = 1; i < mr.curve_n; ++i)
        if (!(mr.curve_t[i] > mr.curve_t[i - 1])) return fail(ctx, TLS_E_ARG, "the template curve's time stamps must ascend");
    if (mr.lc_cap < 1 || mr.lc_cap > 16 * n + 64) return fail(ctx, TLS_E_ARG, "lc_cap out of range [1, 16 n + 64]");
    if (!(mr.maxw >= 1.0) || n > 100000000) return fail(ctx, TLS_E_ARG, "maxw must be at least 1, n at most 1e8");
    return TLS_OK;
}

// the template curve (uploaded once per call), the O(group x n) scratch and results of one group, and the launch shape
int reserve_transit_models(tls_ctx* ctx, const ModelsRequest& mr, int64_t group, int64_t n, ModelsBufs& mb) {
    const T0FitShape shape = t0fit_shape(n);
    mb.resident = shape.resident; mb.nb = shape.nb; mb.lds = shape.lds;
    mb.scratch_stride = (mb.resident ? 0 : 3 * (size_t)n) + 2 * (size_t)tlsdev::kModelsOversample * (size_t)n;
    mb.out_stride = mr.stride(n);
    const size_t g = (size_t)group, curve = 2 * (size_t)mr.curve_n;
    Arena L;
    L.add(mb.curve, curve);   // times | values
    L.add(mb.scratch, g * mb.scratch_stride);  L.add(mb.out, g * mb.out_stride);
    TLS_HIP(ctx, L.bind(ctx->d_models));
    TLS_HIP(ctx, hipMemcpyAsync(mb.curve, mr.curve_t, (size_t)mr.curve_n * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(mb.curve + mr.curve_n, mr.curve_f, (size_t)mr.curve_n * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    return TLS_OK;
}

// the arrays of `gc` curves from the chain's pick and T0 and the statistics stage's epochs, nothing waited for
int enqueue_transit_models(tls_ctx* ctx, const PostSearchBufs& b, const StatsBufs& sb, const StatsRequest& sr,
                           const ModelsRequest& mr, const ModelsBufs& mb, int64_t gc, const double* d_y, int64_t n,
                           double t_min, double t_max) {
    tlsdev::ModelsArgs a;
    a.t = ctx->d_t.ptr; a.y = d_y; a.pick = b.pick; a.T0 = b.T0;
    a.stats = b.stats; a.per_transit = b.per_transit; a.max_epochs = (int)sr.max_epochs;
    a.row_duration = sb.row_duration;
    a.curve_t = mb.curve; a.curve_f = mb.curve + mr.curve_n; a.curve_n = (int)mr.curve_n;
    a.curve_lo = mr.curve_lo; a.curve_hi = mr.curve_hi;
    a.fill_factor = sr.fill_factor; a.t_min = t_min; a.t_max = t_max; a.maxw = mr.maxw;
    a.out = mb.out; a.out_stride = (long long)mb.out_stride; a.lc_cap = mr.lc_cap;
    a.scratch = mb.scratch; a.scratch_stride = (long long)mb.scratch_stride;
    a.n = (int)n; a.nb = mb.nb;
    hipError_t e;
    if (mb.resident) {
        auto kernel = tlsdev::tls_transit_models<true, unsigned short>;
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)mb.lds);
        if (e == hipSuccess) { hipLaunchKernelGGL(kernel, dim3((unsigned)gc), dim3(512), mb.lds, main_stream(ctx), a); e = hipGetLastError(); }
    } else {
        auto kernel = tlsdev::tls_transit_models<false, unsigned int>;
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)mb.lds);
        if (e == hipSuccess) { hipLaunchKernelGGL(kernel, dim3((unsigned)gc), dim3(512), mb.lds, main_stream(ctx), a); e = hipGetLastError(); }
    }
    if (e != hipSuccess) return fail(ctx, TLS_E_HIP, std::string("model launch: ") + hipGetErrorString(e));
    return TLS_OK;
}

// curve c's arrays from the group's host copy (h: `stride` doubles a curve) into the caller's rows; NaN past the model light
// curve's length and in every row of a curve without a fit
int read_transit_models(tls_ctx* ctx, const ModelsRequest& mr, const double* h, size_t stride, int64_t c, int64_t curve,
                        int64_t n) {
    const double* rec = h + stride * (size_t)c;
    const size_t nn = (size_t)n, cap = (size_t)mr.lc_cap;
    double* folded = mr.out_folded + 3 * nn * (size_t)curve;
    double* model = mr.out_model_folded + nn * (size_t)curve;
    double* lc = mr.out_lc + 2 * cap * (size_t)curve;
    const double code = rec[0];
    if (code == tlsdev::kModelsRaises)
        return fail(ctx, TLS_E_ARG, "light curve " + std::to_string((long long)curve) + ": power() raises for its model (" +
                                    std::to_string((long long)rec[1]) + " model samples, or a transit wider than the window)");
    if (code == tlsdev::kModelsTooLong)
        return fail(ctx, TLS_E_ARG, "light curve " + std::to_string((long long)curve) + ": model light curve longer than lc_cap = " +
                                    std::to_string((long long)mr.lc_cap));
    if (code < 0) {
        std::fill(folded, folded + 3 * nn, std::nan("")); std::fill(model, model + nn, std::nan(""));
        std::fill(lc, lc + 2 * cap, std::nan(""));
        mr.out_lc_len[curve] = 0;
        return TLS_OK;
    }
    const size_t len = (size_t)code;
    std::memcpy(folded, rec + tlsdev::kModelsHeader, 3 * nn * 8);
    std::memcpy(model, rec + tlsdev::kModelsHeader + 3 * nn, nn * 8);
    for (int r = 0; r < 2; ++r) {
        std::memcpy(lc + r * cap, rec + tlsdev::kModelsHeader + 4 * nn + r * cap, len * 8);
        std::fill(lc + r * cap + len, lc + (r + 1) * cap, std::nan(""));
    }
    mr.out_lc_len[curve] = (int64_t)len;
    return TLS_OK;
}

// ---- the peaks of the detrended power (tls_power_batch_peaks; tls_find_peaks runs the same kernel on the caller's rows)
struct PeaksRequest {
    int64_t k = 0; double sep = 0; const double* ratios = nullptr; int64_t n_ratios = 0; double min_power = 0;
    tls_peak* out = nullptr; int64_t* out_n = nullptr;
    size_t words() const { return 1 + (size_t)tlsdev::kPeakWords * (size_t)k; }   // n_peaks | k records
};
static_assert(sizeof(tls_peak) == tlsdev::kPeakWords * 8, "tls_peak is the kernel's record");
static_assert(TLS_PEAKS_MAX_K == tlsdev::kPeaksMaxK && TLS_PEAKS_MAX_RATIOS == tlsdev::kPeaksMaxRatios, "the header's limits");

int check_peaks_request(tls_ctx* ctx, const PeaksRequest& pr, int64_t n_periods) {
    if (pr.k < 1 || pr.k > TLS_PEAKS_MAX_K) return fail(ctx, TLS_E_ARG, "peaks: k out of range [1, 32]");
    if (!(std::isfinite(pr.sep) && pr.sep >= 0.0 && pr.sep < 1.0)) return fail(ctx, TLS_E_ARG, "peaks: min_separation must be finite and in [0, 1)");
    if (pr.n_ratios < 0 || pr.n_ratios > TLS_PEAKS_MAX_RATIOS) return fail(ctx, TLS_E_ARG, "peaks: at most 16 ratios");
    if (pr.n_ratios > 0 && !pr.ratios) return fail(ctx, TLS_E_ARG, "peaks: null ratios");
    for (int64_t r = 0; r < pr.n_ratios; ++r)
        if (!(std::isfinite(pr.ratios[r]) && pr.ratios[r] > 0.0)) return fail(ctx, TLS_E_ARG, "peaks: every ratio must be finite and > 0");
    if (std::isnan(pr.min_power)) return fail(ctx, TLS_E_ARG, "peaks: min_power is NaN");
    if (n_periods < 1 || n_periods > tlsdev::kPeaksMaxPeriods) return fail(ctx, TLS_E_ARG, "peaks: n_periods out of range [1, 2^30]");
    return TLS_OK;
}

// the alive masks of `rows` rows in HBM, where a row's mask does not fit the LDS (tls_peaks.hip.h)
int reserve_peak_mask(tls_ctx* ctx, int64_t rows, int64_t n_periods) {
    if (n_periods <= tlsdev::kPeaksLdsPeriods) return TLS_OK;
    TLS_HIP(ctx, ctx->d_peak_mask.reserve((size_t)rows * (size_t)((n_periods + 63) / 64)));
    return TLS_OK;
}

// the peaks of `rows` rows (power at stride power_stride; chi2 / row / depth nullptr or [rows][n_periods]; pick nullptr or the
// records of tls_power_pick) into d_out [rows][words()], nothing waited for
int enqueue_find_peaks(tls_ctx* ctx, const PeaksRequest& pr, int64_t rows, int64_t n_periods, const double* d_power,
                       size_t power_stride, const double* d_periods, const double* d_chi2, const long long* d_row,
                       const double* d_depth, const double* d_pick, double* d_out) {
    tlsdev::PeaksArgs a;
    a.power = d_power; a.power_stride = (long long)power_stride; a.periods = d_periods;
    a.chi2 = d_chi2; a.row = d_row; a.depth = d_depth; a.pick = d_pick;
    a.hbm_mask = ctx->d_peak_mask.ptr; a.out = reinterpret_cast<unsigned long long*>(d_out);
    a.ratios[0] = 1.0;
    for (int64_t r = 0; r < tlsdev::kPeaksMaxRatios; ++r) a.ratios[r + 1] = r < pr.n_ratios ? pr.ratios[r] : 0.0;
    a.sep = pr.sep; a.min_power = pr.min_power; a.n_ratios = (int)pr.n_ratios + 1;
    a.n = (int)n_periods; a.k = (int)pr.k;
    hipError_t e;
    if (n_periods <= tlsdev::kPeaksLdsPeriods) {
        auto kernel = tlsdev::tls_find_peaks<true>;
        const size_t lds = (size_t)((n_periods + 63) / 64) * 8;
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e == hipSuccess) { hipLaunchKernelGGL(kernel, dim3((unsigned)rows), dim3(1024), lds, main_stream(ctx), a); e = hipGetLastError(); }
    } else {
        hipLaunchKernelGGL(tlsdev::tls_find_peaks<false>, dim3((unsigned)rows), dim3(1024), 0, main_stream(ctx), a);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return fail(ctx, TLS_E_HIP, std::string("peaks launch: ") + hipGetErrorString(e));
    return TLS_OK;
}

// row c's peaks from a host copy of the kernel's records (`words()` doubles a row) into the caller's arrays
void read_peaks(const PeaksRequest& pr, const double* h, int64_t c, int64_t curve) {
    const double* rec = h + pr.words() * (size_t)c;
    int64_t n_peaks;
    std::memcpy(&n_peaks, rec, 8);
    pr.out_n[curve] = n_peaks;
    std::memcpy(pr.out + (size_t)curve * (size_t)pr.k, rec + 1, (size_t)pr.k * sizeof(tls_peak));
}

// ---- the phase scan (tls_phase_scan on the caller's candidates; tls_power_batch_phase_scan behind every slab of peak fits):
// one workgroup a fit (tls_phase_scan.hip.h, DESIGN.md "Phase scan")
struct PhaseScanRequest {
    int64_t max_bins = 0, min_count = 0;
    tls_phase_record* out = nullptr;           // [n_fits], or [n_curves][k]
};
static_assert(sizeof(tls_phase_record) == tlsdev::kPhaseWords * 8, "tls_phase_record is the kernel's record");
static_assert(TLS_PHASE_SCAN_MIN_BINS == tlsdev::kPhaseMinBins && TLS_PHASE_SCAN_MAX_BINS == tlsdev::kPhaseMaxBins, "the header's limits");

int check_phase_scan_request(tls_ctx* ctx, const PhaseScanRequest& ps) {
    if (ps.max_bins < TLS_PHASE_SCAN_MIN_BINS || ps.max_bins > TLS_PHASE_SCAN_MAX_BINS)
        return fail(ctx, TLS_E_ARG, "phase scan: max_bins out of range [16, 4096]");
    if (ps.min_count < 1 || ps.min_count > INT32_MAX) return fail(ctx, TLS_E_ARG, "phase scan: min_count < 1");
    return TLS_OK;
}

// the scans of `fits` fits into d_out [fits][12], nothing waited for; fit f reads the flux row d_curve[f] of d_y [..][n],
// d_period[f * period_stride], d_T0[f] and d_duration[f * duration_stride], and is not scanned where d_status[f] != 0
int enqueue_phase_scan(tls_ctx* ctx, const PhaseScanRequest& ps, int64_t fits, const double* d_t, const double* d_y, int64_t n,
                       const int* d_curve, const double* d_period, int period_stride, const double* d_T0,
                       const double* d_duration, int duration_stride, const double* d_status, double* d_out) {
    tlsdev::PhaseScanArgs a;
    a.t = d_t; a.y = d_y; a.curve = d_curve;
    a.period = d_period; a.T0 = d_T0; a.duration = d_duration;
    a.period_stride = period_stride; a.duration_stride = duration_stride;
    a.status = d_status; a.out = d_out;
    a.n = (int)n; a.max_bins = (int)ps.max_bins; a.min_count = (int)ps.min_count;
    auto kernel = tlsdev::tls_phase_scan_kernel;
    const size_t lds = tlsdev::phase_scan_lds_bytes(a.max_bins);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)fits), dim3(tlsdev::kPhaseThreads), lds, main_stream(ctx), a);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return fail(ctx, TLS_E_HIP, std::string("phase scan launch: ") + hipGetErrorString(e));
    return TLS_OK;
}

// ---- the peak-fit stage (tls_power_batch_peak_fits; tls_debug_peak_fits feeds it injected peak records): the final T0 fit
// and the statistics record of EVERY peak of a group, fits f = c k + r in slabs of kPeakFitSlab behind the group's peaks
// kernel, on arrays of its own (tls_peak_fits.hip.h, DESIGN.md "Peak fits")
struct PeakFitsRequest {
    int64_t k = 0;
    const StatsRequest* inputs = nullptr;      // row_duration, fill_factor, root, root_count, max_epochs (its outputs are not read)
    tls_peak_fit* out = nullptr;               // [n_curves][k]
    // tls_debug_peak_fits: every fit's trial epochs and residuals [n_curves][k][n], n_epochs [n_curves][k]
    double* out_epochs = nullptr; double* out_residuals = nullptr; int64_t* out_n_epochs = nullptr;
    size_t words() const { return (size_t)tlsdev::kPeakFitWords * (size_t)k; }
};
static_assert(sizeof(tls_peak_fit) == tlsdev::kPeakFitWords * 8, "tls_peak_fit is T0, status and the statistics record");

struct PeakFitBufs {
    double *pick = nullptr, *per_transit = nullptr, *signal = nullptr, *epochs = nullptr, *residuals = nullptr, *scratch = nullptr;
    tlsdev::T0FitParams* fit = nullptr;
    int *n_epochs = nullptr, *curve = nullptr, *ranges = nullptr;
    size_t fit_stride = 0, scratch_stride = 0;
    int64_t max_len = 1, slab = 1;
};

// the arrays of one slab of fits (device bytes: DESIGN.md "Peak fits" has the formula)
int reserve_peak_fits(tls_ctx* ctx, int64_t fits_total, int64_t n, int64_t max_len, int64_t max_epochs, PeakFitBufs& fb) {
    fb.slab = std::max<int64_t>(1, std::min<int64_t>(tlsdev::kPeakFitSlab, fits_total));
    fb.max_len = std::max<int64_t>(max_len, 1);
    fb.fit_stride = (size_t)n;
    fb.scratch_stride = 4 * (size_t)n + 1;
    const size_t s = (size_t)fb.slab, rows = (size_t)tlsdev::kPerTransitRows * (size_t)max_epochs;
    Arena L;
    L.add(fb.pick, 8 * s);  L.add(fb.per_transit, rows * s);  L.add(fb.signal, (size_t)fb.max_len * s);  L.add(fb.fit, s);
    L.add(fb.n_epochs, 2 * s);   // (a double's room a fit, this and the next)
    L.add(fb.curve, 2 * s);
    TLS_HIP(ctx, L.bind(ctx->d_pfit));
    TLS_HIP(ctx, ctx->d_pfep.reserve(s * fb.fit_stride));
    TLS_HIP(ctx, ctx->d_pfres.reserve(s * fb.fit_stride));
    TLS_HIP(ctx, ctx->d_pfstats.reserve(s * fb.scratch_stride));
    TLS_HIP(ctx, ctx->d_pfranges.reserve(s * 3 * (size_t)max_epochs));
    fb.epochs = ctx->d_pfep.ptr; fb.residuals = ctx->d_pfres.ptr; fb.scratch = ctx->d_pfstats.ptr; fb.ranges = ctx->d_pfranges.ptr;
    return TLS_OK;
}

// the fits of `gc` curves: d_peaks the group's peak records, d_y [gc][n] and d_power (stride power_stride) the curves' flux
// and detrended power, sb the statistics inputs on the device; results into d_out = T0 [cap] | status [cap] | records
// [cap][16], cap = group k.  Nothing waited for, unless the request wants the fits' epochs back (`first_curve`: the batch
// index of the group's first curve in those arrays), which are copied slab by slab.  ps: every fit's phase scan behind its
// slab, from the period of the slab's pick, T0 and duration_days of its record, into d_scans [cap][12].
int enqueue_peak_fits(tls_ctx* ctx, const PeakFitBufs& fb, const PeakFitsRequest& pf, const StatsBufs& sb, int64_t gc,
                      int64_t group, const double* d_peaks, double* d_out, const double* d_y, const double* d_power,
                      size_t power_stride, int64_t n, int64_t n_periods, double t_min, double t_max, double margin,
                      int64_t first_curve = 0, const PhaseScanRequest* ps = nullptr, double* d_scans = nullptr) {
    const StatsRequest& in = *pf.inputs;
    const int64_t total = gc * pf.k, cap = group * pf.k;
    double* T0 = d_out; double* status = d_out + cap; double* stats = d_out + 2 * cap;
    for (int64_t f0 = 0; f0 < total; f0 += fb.slab) {
        const int64_t fits = std::min<int64_t>(fb.slab, total - f0);
        tlsdev::PeakPicksArgs pa;
        pa.peaks = reinterpret_cast<const unsigned long long*>(d_peaks);
        pa.pick = fb.pick; pa.curve = fb.curve; pa.status = status + f0;
        pa.k = (int)pf.k; pa.first = (int)f0; pa.fits = (int)fits;
        hipLaunchKernelGGL(tlsdev::tls_peak_picks, dim3((unsigned)((fits + 255) / 256)), dim3(256), 0, main_stream(ctx), pa);
        tlsdev::PrepArgs pr;
        pr.pick = fb.pick; pr.widths = ctx->d_widths.ptr; pr.n_widths = ctx->plan.n_widths; pr.q = ctx->d_q.ptr;
        pr.signal = fb.signal; pr.signal_stride = (long long)fb.max_len; pr.epochs = fb.epochs; pr.epoch_stride = (long long)fb.fit_stride;
        pr.params = fb.fit; pr.n_epochs = fb.n_epochs; pr.t_min = t_min; pr.margin = margin; pr.n = (int)n;
        hipLaunchKernelGGL(tlsdev::tls_power_prep, dim3((unsigned)fits), dim3(256), 0, main_stream(ctx), pr);
        TLS_HIP(ctx, hipGetLastError());
        int rc = launch_t0_fit(ctx, ctx->d_t.ptr, d_y, fb.signal, fb.epochs, fb.residuals, nullptr, n, 1.0, 0, 0, 0, t_min, t_max,
                               fb.fit, fits, n, fb.max_len, (int64_t)fb.fit_stride, fb.curve);
        if (rc) return rc;
        tlsdev::FirstMinArgs fa;
        fa.residuals = fb.residuals; fa.epochs = fb.epochs; fa.n_epochs = fb.n_epochs;
        fa.T0 = T0 + f0; fa.stride = (long long)fb.fit_stride;
        hipLaunchKernelGGL(tlsdev::tls_first_min, dim3((unsigned)fits), dim3(1024), 0, main_stream(ctx), fa);
        tlsdev::TransitStatsArgs a;
        a.t = ctx->d_t.ptr; a.y = d_y; a.pick = fb.pick; a.T0 = T0 + f0;
        a.power = d_power; a.power_stride = (long long)power_stride; a.curve = fb.curve;
        a.periods = ctx->d_periods.ptr; a.n_periods = (int)n_periods;
        a.row_duration = sb.row_duration; a.root = sb.root; a.root_count = sb.root_count; a.n_root = (int)in.n_root;
        a.fill_factor = in.fill_factor; a.t_min = t_min; a.t_max = t_max;
        a.stats = stats + (size_t)f0 * tlsdev::kTransitStats; a.per_transit = fb.per_transit;
        a.ranges = fb.ranges; a.scratch = fb.scratch; a.scratch_stride = (long long)fb.scratch_stride;
        a.n = (int)n; a.max_epochs = (int)in.max_epochs;
        hipLaunchKernelGGL(tlsdev::tls_transit_stats, dim3((unsigned)fits), dim3(256), 0, main_stream(ctx), a);
        TLS_HIP(ctx, hipGetLastError());
        if (ps && (rc = enqueue_phase_scan(ctx, *ps, fits, ctx->d_t.ptr, d_y, n, fb.curve, fb.pick + 3, 8, T0 + f0,
                                           a.stats + 1, tlsdev::kTransitStats, status + f0,
                                           d_scans + (size_t)f0 * tlsdev::kPhaseWords))) return rc;
        if (pf.out_epochs || pf.out_residuals || pf.out_n_epochs) {
            // (the next slab overwrites these arrays: the copies are done before it is enqueued)
            const size_t at = (size_t)(first_curve * pf.k + f0), bytes = (size_t)fits * fb.fit_stride * 8;
            std::vector<int> nep((size_t)fits);
            if (pf.out_epochs) TLS_HIP(ctx, hipMemcpyAsync(pf.out_epochs + at * fb.fit_stride, fb.epochs, bytes, hipMemcpyDeviceToHost, main_stream(ctx)));
            if (pf.out_residuals) TLS_HIP(ctx, hipMemcpyAsync(pf.out_residuals + at * fb.fit_stride, fb.residuals, bytes, hipMemcpyDeviceToHost, main_stream(ctx)));
            TLS_HIP(ctx, hipMemcpyAsync(nep.data(), fb.n_epochs, (size_t)fits * sizeof(int), hipMemcpyDeviceToHost, main_stream(ctx)));
            TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));
            if (pf.out_n_epochs) for (int64_t l = 0; l < fits; ++l) pf.out_n_epochs[at + (size_t)l] = nep[(size_t)l];
        }
    }
    return TLS_OK;
}

// the k fits of curve c from the group's host copy (enqueue_peak_fits' layout); TLS_E_ARG for a candidate whose row starts
// no template duration (tls_power_prep's finding) or that has more than max_epochs epochs, as the main chain reports its pick
int read_peak_fits(tls_ctx* ctx, const PeakFitsRequest& pf, const double* h, int64_t group, int64_t c, int64_t curve) {
    const size_t cap = (size_t)group * (size_t)pf.k;
    for (int64_t r = 0; r < pf.k; ++r) {
        const size_t f = (size_t)(c * pf.k + r);
        const double status = h[cap + f];
        const double* rec = h + 2 * cap + f * (size_t)tlsdev::kTransitStats;
        const std::string who = "peak " + std::to_string((long long)r) + " of light curve " + std::to_string((long long)curve);
        // (tls_power_prep found no template width starting at the row and raised the pick's [7]: the statistics kernel left
        // the record of a pick without fit)
        if (status == tlsdev::kPeakFitted && std::isnan(rec[10]))
            return fail(ctx, TLS_E_ARG, "the template row of " + who + " is not the first row of a duration");
        tls_peak_fit& o = pf.out[(size_t)curve * (size_t)pf.k + (size_t)r];
        o.status = status;
        if (status != tlsdev::kPeakFitted) {
            double* d = reinterpret_cast<double*>(&o.stats);
            o.T0 = std::nan("");
            std::fill(d, d + tlsdev::kTransitStats, std::nan(""));
            continue;
        }
        if (rec[10] > (double)pf.inputs->max_epochs)
            return fail(ctx, TLS_E_ARG, who + " has more than max_epochs = " + std::to_string((long long)pf.inputs->max_epochs) +
                                        " transit epochs");
        o.T0 = h[f];
        std::memcpy(&o.stats, rec, sizeof(tls_transit_stats));
    }
    return TLS_OK;
}

// the summary of curve c from the chain's results on the host (sde | pick | T0 of `group` curves, as reserve_post_search
// lays them out); TLS_E_ARG when tls_power_prep found no template width starting at the picked row
int read_summary(tls_ctx* ctx, const double* h_sde, int64_t group, int64_t c, int64_t curve, tls_power_summary& os) {
    const double* pk = h_sde + 2 * group + 8 * c;
    const double T0 = h_sde[10 * group + c];
    if (pk[7] != 0.0)
        return fail(ctx, TLS_E_ARG, "template row " + std::to_string((long long)pk[5]) + " at the chi2 minimum of light curve " +
                                    std::to_string((long long)curve) + " is not the first row of a duration");
    const bool no_fit = pk[6] != 0.0;
    os.chi2_min = pk[0]; os.index_best = (int64_t)pk[1]; os.index_power = (int64_t)pk[2];
    os.best_row = (int64_t)pk[5]; os.no_fit = no_fit ? 1 : 0;
    if (no_fit) {   // main.py:216-267: flat spectra
        os.SDE = 0; os.SDE_raw = 0; os.period = std::nan(""); os.T0 = 0; os.depth = 1;
    } else {
        os.SDE_raw = h_sde[2 * c]; os.SDE = h_sde[2 * c + 1]; os.period = pk[3]; os.depth = pk[4]; os.T0 = T0;
    }
    return TLS_OK;
}

// ---- survey batches (tls_search_batch, tls_power_batch*): groups of up to `group` light curves, ONE search launch each
using BatchSlot = tls_ctx::BatchSlot;

// the events and the pinned staging of both slots: a group's flux in (stage_group's layout), `out_doubles` of results out
int reserve_batch_staging(tls_ctx* ctx, int64_t group, size_t nn, size_t out_doubles) {
    const size_t in_doubles = (size_t)group * nn * (ctx->plan.uniform ? 1 : 2) + 2 * (size_t)group;
    auto grow = [ctx](double*& buf, size_t& cap, size_t doubles) -> int {
        if (cap >= doubles) return TLS_OK;
        if (buf) TLS_HIP(ctx, hipHostFree(buf));
        buf = nullptr; cap = 0;
        TLS_HIP(ctx, hipHostMalloc(reinterpret_cast<void**>(&buf), doubles * 8, hipHostMallocDefault));
        cap = doubles;
        return TLS_OK;
    };
    for (auto& sl : ctx->slot) {
        for (hipEvent_t* ev : {&sl.ev_in, &sl.ev_kernel, &sl.ev_out})
            if (!*ev) TLS_HIP(ctx, hipEventCreateWithFlags(ev, hipEventDisableTiming));
        int rc = grow(sl.h_in, sl.h_in_cap, in_doubles);
        if (rc || (rc = grow(sl.h_out, sl.h_out_cap, out_doubles))) return rc;
    }
    return TLS_OK;
}

// a slot's device buffers for one group: flux (weights), per-curve constants, search results
int reserve_batch_slot(tls_ctx* ctx, BatchSlot& sl, int64_t group, size_t nn, size_t np) {
    const size_t g = (size_t)group;
    TLS_HIP(ctx, sl.d_y.reserve(g * nn));
    if (!ctx->plan.uniform) TLS_HIP(ctx, sl.d_w.reserve(g * nn));
    TLS_HIP(ctx, sl.d_S0.reserve(g));
    TLS_HIP(ctx, sl.d_w0.reserve(g));
    TLS_HIP(ctx, sl.d_chi2.reserve(g * np));
    TLS_HIP(ctx, sl.d_row.reserve(g * np));
    TLS_HIP(ctx, sl.d_depth.reserve(g * np));
    return TLS_OK;
}

// a group formed in a slot's pinned h_in (y | w, per-point dy only | S0 | w0; `group` curves each) and what its launch needs
struct GroupState {
    int64_t gc = 0;
    double *y = nullptr, *w = nullptr, *S0 = nullptr, *w0 = nullptr;
    double sigma_sum = 0, y_max = 0, e_max = 0;   // flux_scatter summed over the curves; largest |y| and |1 - y| (weights_from)
};

// host side of the group of curves c0 .. c0 + gc: flux, weights, S0 (core.py:127)
int stage_group(tls_ctx* ctx, BatchSlot& sl, const double* y, const double* dy, int64_t n, int64_t c0, int64_t gc, int64_t group,
                GroupState& st) {
    const size_t nn = (size_t)n;
    const bool uni = ctx->plan.uniform;
    st = GroupState{};
    st.gc = gc;
    st.y = sl.h_in; st.w = sl.h_in + (size_t)group * nn;
    st.S0 = sl.h_in + (size_t)group * nn * (uni ? 1 : 2); st.w0 = st.S0 + group;
    std::vector<double> w;
    for (int64_t c = 0; c < gc; ++c) {
        const double* yc = y + (c0 + c) * n;
        bool uniform; double w0, S0;
        weights_from(yc, dy + (c0 + c) * n, n, uniform, w0, w, S0, &st.y_max, &st.e_max);
        if (uniform != uni) return fail(ctx, TLS_E_ARG, "light curves of a batch must all have uniform or all have per-point dy");
        st.S0[c] = S0; st.w0[c] = w0;
        std::memcpy(st.y + (size_t)c * nn, yc, nn * 8);
        if (!uniform) std::memcpy(st.w + (size_t)c * nn, w.data(), nn * 8);
        st.sigma_sum += flux_scatter(yc, n);
    }
    return TLS_OK;
}

// the staged group up to a slot's device buffers, on `stream`
int upload_group(tls_ctx* ctx, BatchSlot& sl, const GroupState& st, size_t nn, hipStream_t stream) {
    const size_t gc = (size_t)st.gc;
    TLS_HIP(ctx, hipMemcpyAsync(sl.d_y.ptr, st.y, gc * nn * 8, hipMemcpyHostToDevice, stream));
    if (!ctx->plan.uniform) TLS_HIP(ctx, hipMemcpyAsync(sl.d_w.ptr, st.w, gc * nn * 8, hipMemcpyHostToDevice, stream));
    TLS_HIP(ctx, hipMemcpyAsync(sl.d_S0.ptr, st.S0, gc * 8, hipMemcpyHostToDevice, stream));
    TLS_HIP(ctx, hipMemcpyAsync(sl.d_w0.ptr, st.w0, gc * 8, hipMemcpyHostToDevice, stream));
    return TLS_OK;
}

// enqueue() back on the context's own buffers
void unbind_batch_slot(tls_ctx* ctx) {
    ctx->batch_curves = 1;
    ctx->over_y = ctx->over_w = ctx->over_S0 = ctx->over_w0 = nullptr;
    ctx->over_chi2 = nullptr; ctx->over_row = nullptr; ctx->over_depth = nullptr;
}

// ONE search launch over a staged group whose flux is on slot sl (the fold + sort of a period is shared by the group's curves);
// the context points at the slot for this call only, whichever way it returns
int search_group(tls_ctx* ctx, BatchSlot& sl, const GroupState& st) {
    ctx->S0 = st.S0[0]; ctx->w0 = st.w0[0]; ctx->y_abs_max = st.y_max; ctx->e_abs_max = st.e_max;
    choose_flux_kernels(ctx, st.sigma_sum / (double)st.gc);
    struct Unbind { tls_ctx* ctx; ~Unbind() { unbind_batch_slot(ctx); } } unbind{ctx};
    ctx->batch_curves = (int)st.gc;
    ctx->over_y = sl.d_y.ptr; ctx->over_w = ctx->plan.uniform ? nullptr : sl.d_w.ptr; ctx->over_S0 = sl.d_S0.ptr; ctx->over_w0 = sl.d_w0.ptr;
    ctx->over_chi2 = sl.d_chi2.ptr; ctx->over_row = sl.d_row.ptr; ctx->over_depth = sl.d_depth.ptr;
    return enqueue(ctx, false);
}

// the one failure exit of both batch entries: nothing still copies into or out of the pinned slots or the caller's arrays
// (asynchronous copies may be in flight on either stream), no launch override survives, and the context holds no results
int end_batch(tls_ctx* ctx, int rc) {
    if (ctx && rc != TLS_OK) {
        (void)hipStreamSynchronize(main_stream(ctx));
        if (ctx->copy_stream) (void)hipStreamSynchronize(ctx->copy_stream);
        unbind_batch_slot(ctx);
        ctx->executed = false;
    }
    return rc;
}

// compute units of the first visible device; 256 (MI355X) where no device can be asked (host-only planning)
int visible_compute_units() {
    static int cached = 0;
    if (cached > 0) return cached;
    int count = 0, cus = 0;
    if (hipGetDeviceCount(&count) == hipSuccess && count > 0 &&
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0) == hipSuccess && cus > 0) cached = cus;
    else { (void)hipGetLastError(); cached = 256; }
    return cached;
}

// ---- the duration rows of tls_single.hip.h and their taps, as tls_single_transits, tls_transit_times and
// tls_event_vetting read them
struct RowTables {
    std::vector<tlsdev::SingleRow> rows;
    std::vector<double> taps;      // pairs (b, b * b)
    std::vector<double> slopes;    // on request: triples (g, b * g, g * g), g the shape's slope per sample
    size_t n_taps = 0;
};

int build_row_tables(tls_ctx* ctx, const std::string& what, const char* null_text, const double* shape_values,
                     const int64_t* shape_offset, const int64_t* width, const double* span_max, int64_t n_rows, bool with_slopes,
                     RowTables& tb) {
    if (n_rows < 1) return fail(ctx, TLS_E_ARG, what + ": at least one row is needed");
    if (!shape_values || !shape_offset || !width || !span_max) return fail(ctx, TLS_E_ARG, null_text);
    if (n_rows > TLS_SINGLE_MAX_WIDTH) return fail(ctx, TLS_E_ARG, what + ": more rows than widths there are");
    for (int64_t r = 0; r < n_rows; ++r) {
        if (width[r] < tlsdev::kSingleMinWidth || width[r] > TLS_SINGLE_MAX_WIDTH)
            return fail(ctx, TLS_E_ARG, what + ": width out of range [3, 4096]");
        if (r > 0 && width[r] <= width[r - 1]) return fail(ctx, TLS_E_ARG, what + ": the widths must be strictly ascending");
        if (shape_offset[r] < 0) return fail(ctx, TLS_E_ARG, what + ": negative shape offset");
        if (!(std::isfinite(span_max[r]) && span_max[r] >= 0.0)) return fail(ctx, TLS_E_ARG, what + ": span_max must be finite and >= 0");
        tb.n_taps += (size_t)width[r];
    }
    tb.rows.resize((size_t)n_rows);
    tb.taps.resize(2 * tb.n_taps);
    tb.slopes.resize(with_slopes ? 3 * tb.n_taps : 0);
    size_t at = 0;
    for (int64_t r = 0; r < n_rows; ++r) {
        tb.rows[(size_t)r].width = (int)width[r];
        tb.rows[(size_t)r].offset = (int)at;
        tb.rows[(size_t)r].span_max = span_max[r];
        const double* b = shape_values + shape_offset[r];
        for (int64_t j = 0; j < width[r]; ++j, ++at) {
            const double v = b[j];
            tb.taps[2 * at] = v;
            tb.taps[2 * at + 1] = v * v;
            if (!with_slopes) continue;
            const double next = j + 1 < width[r] ? b[j + 1] : 0.0, prev = j > 0 ? b[j - 1] : 0.0;
            const double rise = next - prev;
            const double g = 0.5 * rise;
            tb.slopes[3 * at] = g;
            tb.slopes[3 * at + 1] = v * g;
            tb.slopes[3 * at + 2] = g * g;
        }
    }
    return TLS_OK;
}

// ---- candidate slabs (tls_candidate_slabs.h, DESIGN.md "Candidate slabs"): the loop the per-candidate stages share
struct SlabCopy { double* dev; const double* host; };          // an array of one slab and the caller's whole array (null: not given)
struct SlabView { int64_t f0; size_t fits, curves, lds; };     // lds: the largest dynamic LDS size the pack hook asked for

struct SlabStage {
    const char* what;              // "transit times": starts the messages
    const char* kernel;            // what tls_last_kernel reports
    const int64_t* curve;
    int64_t n_fits;
    size_t n;
    size_t cs, sl;                 // curves and candidates of one slab at most: the stage's memory statement
    std::vector<SlabCopy> rows;    // curve rows, [cs][n] of [n_curves][n]: one copy per run
    std::vector<SlabCopy> columns; // per-candidate values, [sl] of [n_fits]
    int* d_ints;                   // slot | the pack hook's columns, each sl long
    size_t int_columns;
};

// Walks the slabs of a stage.  pack(f, at) fills candidate f's further integer columns (at[sl], at[2 * sl], ...) and returns
// the dynamic LDS its workgroup needs; launch(slab) enqueues the stage's kernels and checks nothing; fetch(slab) enqueues
// the copies back.
template <typename Pack, typename Launch, typename Fetch>
int run_candidate_slabs(tls_ctx* ctx, const SlabStage& st, Pack pack, Launch launch, Fetch fetch) {
    std::vector<int> h_ints(st.int_columns * st.sl);
    tlsslab::Slab slab;
    for (int64_t f0 = 0; f0 < st.n_fits; f0 += (int64_t)slab.fits) {
        tlsslab::next_slab(st.curve, st.n_fits, f0, st.cs, st.sl, h_ints.data(), slab);
        SlabView s{f0, slab.fits, slab.curves, 0};
        for (size_t i = 0; i < s.fits; ++i) s.lds = std::max<size_t>(s.lds, pack(f0 + (int64_t)i, &h_ints[i]));
        for (const tlsslab::Run& run : slab.runs)
            for (const SlabCopy& r : st.rows)
                if (r.host) TLS_HIP(ctx, hipMemcpyAsync(r.dev + run.slot * st.n, r.host + (size_t)run.curve * st.n, run.count * st.n * 8, hipMemcpyHostToDevice, main_stream(ctx)));
        const size_t ints = st.int_columns > 1 ? st.int_columns * st.sl : s.fits;
        TLS_HIP(ctx, hipMemcpyAsync(st.d_ints, h_ints.data(), ints * sizeof(int), hipMemcpyHostToDevice, main_stream(ctx)));
        for (const SlabCopy& c : st.columns)
            if (c.host) TLS_HIP(ctx, hipMemcpyAsync(c.dev, c.host + f0, s.fits * 8, hipMemcpyHostToDevice, main_stream(ctx)));
        launch(s);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(main_stream(ctx));
            return fail(ctx, TLS_E_HIP, std::string(st.what) + " launch: " + hipGetErrorString(e));
        }
        ctx->last_kernel = st.kernel;
        if (int rc = fetch(s)) return rc;
        // (the next slab overwrites the device buffers and h_ints; what a stage uploaded before the loop is read until the
        // stream is done)
        TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));
    }
    return TLS_OK;
}

const auto no_int_columns = [](int64_t, int*) { return (size_t)0; };

// the pairs kernel of tls_times.hip.h over the first `curves` slots of a slab; false: the launch failed (the error stays
// for hipGetLastError) and the stage's own kernel is not to follow
bool launch_times_pairs(tls_ctx* ctx, tlsdev::TimesPairsArgs p, size_t curves, size_t n) {
    p.count = (long long)(curves * n);
    const unsigned blocks = (unsigned)std::min<long long>((p.count + tlsdev::kTimesThreads - 1) / tlsdev::kTimesThreads, 8192);
    hipLaunchKernelGGL(tlsdev::tls_times_pairs_kernel, dim3(blocks), dim3(tlsdev::kTimesThreads), 0, main_stream(ctx), p);
    return hipPeekAtLastError() == hipSuccess;
}

}  // namespace

extern "C" {

const char* tls_version(void) { return "tls_amd 0.4 (gfx950)"; }

int tls_abi_version(void) { return TLS_AMD_ABI_VERSION; }

int tls_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { g_create_error = std::string("hipGetDeviceCount: ") + hipGetErrorString(e); return TLS_E_HIP; }
    return n;
}

const char* tls_last_error(const tls_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

const char* tls_device_name(const tls_ctx* ctx) { return ctx ? ctx->name.c_str() : ""; }

tls_ctx* tls_ctx_create(int device_id) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        g_create_error = std::string("no usable GPU (hipGetDeviceCount: ") + hipGetErrorString(e) +
                         "); this library has no CPU fallback";
        return nullptr;
    }
    if (device_id < 0 || device_id >= n) {
        g_create_error = "device_id " + std::to_string(device_id) + " out of range (" + std::to_string(n) + " GPUs)";
        return nullptr;
    }
    tls_ctx* ctx = new (std::nothrow) tls_ctx();
    if (!ctx) { g_create_error = "out of host memory"; return nullptr; }
    ctx->device = device_id;
    ctx->opt = process_options();
    hipDeviceProp_t prop;
    if ((e = hipSetDevice(device_id)) != hipSuccess || (e = hipGetDeviceProperties(&prop, device_id)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&ctx->lane_a_stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipEventCreate(&ctx->ev0)) != hipSuccess || (e = hipEventCreate(&ctx->ev1)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&ctx->ev_state, hipEventDisableTiming)) != hipSuccess) {
        g_create_error = std::string("context setup: ") + hipGetErrorString(e);
        delete ctx;
        return nullptr;
    }
    ctx->n_cu = prop.multiProcessorCount;
    char buf[256];
    std::snprintf(buf, sizeof buf, "%s %s, %d CUs, %.0f GiB", prop.gcnArchName, prop.name, ctx->n_cu,
                  (double)prop.totalGlobalMem / (1024.0 * 1024.0 * 1024.0));
    ctx->name = buf;
    return ctx;
}

int tls_get_options(const tls_ctx* ctx, tls_options* out) {
    if (!ctx || !out) return TLS_E_ARG;
    out->exact_prefix = ctx->opt.exact_prefix; out->slim = ctx->opt.slim;
    return TLS_OK;
}

namespace {
int adopt_switches(tls_ctx* ctx, const Switches& o) {
    if (std::memcmp(&o, &ctx->opt, sizeof o) == 0) return TLS_OK;
    ctx->opt = o;
    // a prepared plan was built for the old switches: the next tls_prepare plans again (the key holds them too)
    ctx->prepared = false; ctx->executed = false;
    return TLS_OK;
}
}  // namespace

int tls_set_options(tls_ctx* ctx, const tls_options* opt) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (!opt) return fail(ctx, TLS_E_ARG, "null options");
    Switches o = ctx->opt;
    o.exact_prefix = opt->exact_prefix < 0 ? -1 : opt->exact_prefix;
    o.slim = opt->slim < 0 ? -1 : opt->slim;
    return adopt_switches(ctx, o);
}

int tls_debug_set_switch(tls_ctx* ctx, const char* name, double value) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (name && std::strcmp(name, "lanes") == 0) {
        // launch lanes on (default) or off: where a launch runs, never what it computes -- not a planning switch, so it is
        // no part of the plan key, of tls_debug_get_switches' text or of the environment; changing it joins the lanes
        const int v = value < 0 ? -1 : (int)value;
        if (v != ctx->lanes) { (void)main_stream(ctx); ctx->lanes = v; }
        return TLS_OK;
    }
    const SwitchName* sw = find_switch(name);
    if (!sw) return fail(ctx, TLS_E_ARG, std::string("unknown switch: ") + (name ? name : "(null)"));
    Switches o = ctx->opt;
    switch_store(o, *sw, value);
    return adopt_switches(ctx, o);
}

int tls_debug_get_switches(const tls_ctx* ctx, char* out, int64_t capacity) {
    if (!out || capacity < 1) return TLS_E_ARG;
    const Switches& o = ctx ? ctx->opt : process_options();
    std::string text;
    for (const auto& sw : kSwitchNames) {
        char item[96];
        std::snprintf(item, sizeof item, "%s%s=%.17g", text.empty() ? "" : ",", sw.name, switch_load(o, sw));
        text += item;
    }
    if ((int64_t)text.size() + 1 > capacity) return TLS_E_ARG;
    std::memcpy(out, text.c_str(), text.size() + 1);
    return TLS_OK;
}

void tls_ctx_destroy(tls_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->comm) (void)ncclCommDestroy(ctx->comm);
    if (ctx->lane_b.stream) (void)hipStreamSynchronize(ctx->lane_b.stream);
    if (ctx->lane_a_stream) (void)hipStreamSynchronize(ctx->lane_a_stream);
    ctx->pool.release_all();   // every device buffer of the context, lane B's and the batch slots' included
    {
        auto& lb = ctx->lane_b;
        if (lb.h_stage) (void)hipHostFree(lb.h_stage);
        if (lb.ev_stage) (void)hipEventDestroy(lb.ev_stage);
        if (lb.ev_done) (void)hipEventDestroy(lb.ev_done);
        if (lb.stream) (void)hipStreamDestroy(lb.stream);
    }
    if (ctx->ev_state) (void)hipEventDestroy(ctx->ev_state);
    if (ctx->h_stage) (void)hipHostFree(ctx->h_stage);
    if (ctx->h_out) (void)hipHostFree(ctx->h_out);
    if (ctx->ev_stage) (void)hipEventDestroy(ctx->ev_stage);
    if (ctx->h_band) (void)hipHostFree(ctx->h_band);
    for (auto& ev : ctx->ev_band) if (ev) (void)hipEventDestroy(ev);
    for (auto& sl : ctx->slot) {
        if (sl.h_in) (void)hipHostFree(sl.h_in);
        if (sl.h_out) (void)hipHostFree(sl.h_out);
        if (sl.ev_in) (void)hipEventDestroy(sl.ev_in);
        if (sl.ev_kernel) (void)hipEventDestroy(sl.ev_kernel);
        if (sl.ev_out) (void)hipEventDestroy(sl.ev_out);
    }
    if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
    for (auto& evp : ctx->ev_pool) { (void)hipEventDestroy(evp.first); (void)hipEventDestroy(evp.second); }
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->lane_a_stream) (void)hipStreamDestroy(ctx->lane_a_stream);
    delete ctx;
}

namespace {
// the device buffers the launches of ctx->plan need beside the plan arrays, and the results
int reserve_plan_buffers(tls_ctx* ctx) {
    const SearchPlan& plan = ctx->plan;
    if (plan.split) {
        TLS_HIP(ctx, ctx->d_partials.reserve(3 * (size_t)plan.split_max_items + 3));
        // [split_batch] tiles done | [split_batch] fold ready: all zero between launches (the kernel resets them)
        if (ctx->d_tiles_done.cap < 2 * (size_t)plan.split_batch) {
            TLS_HIP(ctx, ctx->d_tiles_done.reserve(2 * (size_t)plan.split_batch));
            TLS_HIP(ctx, hipMemsetAsync(ctx->d_tiles_done.ptr, 0, ctx->d_tiles_done.cap * sizeof(unsigned int), main_stream(ctx)));
        }
    }
    if (!plan.resident) TLS_HIP(ctx, ctx->d_scratch.reserve(plan.scratch_doubles));
    // three arrays per workgroup: the live units, (pruning) the bound of each, and the units the bound keeps
    TLS_HIP(ctx, ctx->d_lists.reserve((size_t)std::max(std::max(plan.blocks, plan.slim_blocks), plan.split ? plan.split_blocks : 0) * 3 * plan.list_stride));
    if (plan.slim_blocks > 0) TLS_HIP(ctx, ctx->d_perm.reserve(perm_scratch_words(ctx, (size_t)plan.n)));   // (band resolution stashes the order of a period)
    // the table of folded orders of a four-slot plan, within its budget; a plan without one sorts in every launch
    size_t want = plan.perm_table_want;
    if (want > ctx->d_perm_table.cap && ctx->d_perm_table.reserve(want) != hipSuccess) {
        (void)hipGetLastError();   // (no room on the device: not an error)
        ctx->d_perm_table.release();
        want = 0;
    }
    ctx->perm_table_entries = want;
    // results [chi2 | row | depth | counters[4]]
    const size_t np = (size_t)plan.n_periods;
    TLS_HIP(ctx, ctx->d_out.reserve(3 * np + 4));
    point_results(ctx, 0);
    TLS_HIP(ctx, ctx->d_queue.reserve(1));
    if (!ctx->d_squeue.ptr) {   // zero once per context: the kernel rewinds its queue itself
        TLS_HIP(ctx, ctx->d_squeue.reserve(4));   // [0..1] the search (or fold) kernel's queue, [2..3] the split path's search kernel
        TLS_HIP(ctx, hipMemsetAsync(ctx->d_squeue.ptr, 0, 4 * sizeof(unsigned int), main_stream(ctx)));
    }
    return TLS_OK;
}

// the plan arrays of ctx->plan on the device
int stage_plan(tls_ctx* ctx, const double* t, const double* y, const std::vector<double>& w, const double* periods,
               const std::vector<int>& order, const std::vector<tlsdev::PeriodRows>& prow,
               const std::vector<tlsdev::WidthEntry>& widths, const std::vector<double>& q) {
    // ONE pinned staging buffer, ONE device allocation, ONE asynchronous copy; nothing is waited for here (the
    // staging buffer is reused only after its event)
    std::vector<tlsdev::RowScreen> screens;
    build_screens(widths, q, screens, ctx->opt.no_screen == 1);
    const bool uniform = ctx->plan.uniform;
    PlanLayout& L = ctx->layout;
    size_t off = 0;
    auto place = [&](size_t bytes) { const size_t at = off; off = (off + bytes + 255) / 256 * 256; return at; };
    const size_t nn = (size_t)ctx->plan.n, np = (size_t)ctx->plan.n_periods, nw = widths.size(), nq = q.size();
    L.t = place(nn * 8); L.y = place(nn * 8); L.w = place(uniform ? 0 : nn * 8);
    L.periods = place(np * 8); L.order = place(np * sizeof(int)); L.rows = place(np * sizeof(tlsdev::PeriodRows));
    L.widths = place(nw * sizeof(tlsdev::WidthEntry)); L.screens = place(nw * sizeof(tlsdev::RowScreen));
    L.q = place(nq * 8); L.q2 = place(nq * 8);   // (uniform weights: the fp32 rows of the screen instead of q^2)
    const bool with_g = !ctx->plan.resident || ctx->plan.slim_blocks > 0;   // the difference taps: dot products on X (HBM slab; four-slot kernel)
    L.g = place(with_g ? nq * 8 : 0);
    const bool with_tiles = !ctx->plan.resident && ctx->plan.split;
    L.tile_prefix = place(with_tiles ? (np + 1) * sizeof(unsigned int) : 0);
    L.total = off;
    int rcs = stage_reserve(ctx, L.total);
    if (rcs) return rcs;
    TLS_HIP(ctx, ctx->d_plan.reserve(L.total));
    unsigned char* h = ctx->h_stage;
    std::memcpy(h + L.t, t, nn * 8);
    std::memcpy(h + L.y, y, nn * 8);
    if (!uniform) std::memcpy(h + L.w, w.data(), nn * 8);
    if (np) {
        std::memcpy(h + L.periods, periods, np * 8);
        std::memcpy(h + L.order, order.data(), np * sizeof(int));
        std::memcpy(h + L.rows, prow.data(), np * sizeof(tlsdev::PeriodRows));
    }
    std::memcpy(h + L.widths, widths.data(), nw * sizeof(tlsdev::WidthEntry));
    std::memcpy(h + L.screens, screens.data(), nw * sizeof(tlsdev::RowScreen));
    std::memcpy(h + L.q, q.data(), nq * 8);
    ctx->q_count = (long long)nq;
    if (!uniform) {
        double* q2 = reinterpret_cast<double*>(h + L.q2);
        for (size_t j = 0; j < nq; ++j) q2[j] = q[j] * q[j];
    } else {
        float* q32 = reinterpret_cast<float*>(h + L.q2);   // [nq] the rows | [nq] the rows one element later
        for (size_t j = 0; j < nq; ++j) { q32[j] = (float)q[j]; q32[nq + j] = j ? (float)q[j - 1] : 0.0f; }
    }
    if (with_g) {
        // Difference taps of every row, same offsets: g_0 = -q_0, g_j = q_{j-1} - q_j, g_L = q_{L-1}.  With e_k =
        // X_{k+1} - X_k (X the running sum of e) a window's dot product is  sum_j q_j e_{i+j} = sum_{j<=L} g_j X_{i+j}
        // (summation by parts): the slab variant's fast mode evaluates it on the X a tile already holds in LDS for
        // the depth predicate, instead of staging the tile's samples a second time (tls_search_body.inc.h, x_dot).
        double* gt = reinterpret_cast<double*>(h + L.g);
        std::memset(gt, 0, nq * 8);
        for (const auto& we : widths) {
            const double* qr = q.data() + we.q_offset;
            double* gr = gt + we.q_offset;
            gr[0] = -qr[0];
            for (int j = 1; j < we.q_len; ++j) gr[j] = qr[j - 1] - qr[j];
            gr[we.q_len] = qr[we.q_len - 1];
        }
    }
    if (with_tiles) {
        std::memcpy(h + L.tile_prefix, ctx->plan.tile_prefix.data(), (np + 1) * sizeof(unsigned int));
    }
    unsigned char* d = ctx->d_plan.ptr;
    ctx->d_tile_prefix.ptr = reinterpret_cast<unsigned int*>(d + L.tile_prefix);
    ctx->d_t.ptr = reinterpret_cast<double*>(d + L.t); ctx->d_y_a.ptr = reinterpret_cast<double*>(d + L.y);
    ctx->d_y.ptr = ctx->d_y_a.ptr; ctx->flux_lane = 0; ctx->a_reads_flux_b = false;   // (the plan's flux is lane A's)
    ctx->d_w.ptr = reinterpret_cast<double*>(d + L.w); ctx->d_periods.ptr = reinterpret_cast<double*>(d + L.periods);
    ctx->d_order.ptr = reinterpret_cast<int*>(d + L.order); ctx->d_rows.ptr = reinterpret_cast<tlsdev::PeriodRows*>(d + L.rows);
    ctx->d_widths.ptr = reinterpret_cast<tlsdev::WidthEntry*>(d + L.widths);
    ctx->d_screens.ptr = reinterpret_cast<tlsdev::RowScreen*>(d + L.screens);
    ctx->d_q.ptr = reinterpret_cast<double*>(d + L.q); ctx->d_q2.ptr = reinterpret_cast<double*>(d + L.q2);
    ctx->d_g.ptr = reinterpret_cast<double*>(d + L.g);
    TLS_HIP(ctx, hipMemcpyAsync(d, h, L.total, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipEventRecord(ctx->ev_stage, main_stream(ctx)));
    ctx->stage_pending = true;
    return TLS_OK;
}
}  // namespace

int tls_prepare(tls_ctx* ctx, const double* t, const double* y, const double* dy, int64_t n,
                const double* periods, int64_t n_periods, const tls_template* tmpl, const tls_params* params) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    ctx->prepared = false; ctx->executed = false;
    if (!t || !y || !dy || !periods || !tmpl || !params) return fail(ctx, TLS_E_ARG, "null argument");
    if (n < 3 || n > 50000000) return fail(ctx, TLS_E_ARG, "n out of range (need 3 <= n <= 5e7)");
    if (n_periods < 0 || n_periods > 100000000) return fail(ctx, TLS_E_ARG, "n_periods out of range");
    if (tmpl->n_rows < 1 || !tmpl->values || !tmpl->offset || !tmpl->length || !tmpl->width || !tmpl->overshoot)
        return fail(ctx, TLS_E_ARG, "empty template table");
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    (void)main_stream(ctx);   // (tls_prepare always joins the lanes: the flux goes to lane A, the next search starts there)

    // The same time stamps, periods, template and parameters as the plan this context already holds (a survey, or
    // repeated power() calls): only the flux is new.  tls_prepare then costs two passes over y and one upload.
    if (ctx->key.valid && key_matches(ctx->key, ctx->opt, t, n, periods, n_periods, tmpl, params)) {
        const int rcu = update_flux_impl(ctx, y, dy);
        if (rcu == TLS_OK) { ctx->prepared = true; ++ctx->plan_reuses; return TLS_OK; }
        if (rcu != kWeightsDiffer) return rcu;
        // uniform dy after per-point dy (or the reverse): a different kernel variant and layout -- plan again
    }
    ctx->key.valid = false;
    ctx->perm_filled = false; ctx->perm_filled_before_prev = false; ctx->perm_table_entries = 0;   // (the table of folded orders belongs to the key)

    std::vector<tlsdev::WidthEntry> widths;
    std::vector<double> q;
    { int rcw = build_widths(ctx, tmpl, params, n, widths, &q); if (rcw) return rcw; }
    const int64_t M = n + padded_width(widths);
    if (M + 1 > 0x7fffffff / 4) return fail(ctx, TLS_E_ARG, "series too long");
    if (M < 4 * tlsdev::kR) return fail(ctx, TLS_E_ARG, "series too short (need n + widest width >= 20 samples)");

    // per-period duration window (core.py:143-156) and cost
    double t_min, t_max;
    time_range(t, n, t_min, t_max);
    std::vector<tlsdev::PeriodRows> prow((size_t)n_periods);
    std::vector<int64_t> cost((size_t)n_periods);
    GridPlan gp;
    if (!plan_periods(widths, params, periods, n_periods, t_max - t_min, n, M, prow.data(), cost.data(), &gp, ctx->opt.plan_threads))
        return fail(ctx, TLS_E_ARG, "periods must be positive and finite");
    // weights
    std::vector<double> w;
    bool uniform; double w0, S0;
    double y_abs_max = 0.0, e_abs_max = 0.0;
    weights_from(y, dy, n, uniform, w0, w, S0, &y_abs_max, &e_abs_max);
    ctx->y_abs_max = y_abs_max; ctx->e_abs_max = e_abs_max;
    const double flux_sigma = flux_scatter(y, n);

    std::vector<int> order;
    order_queue(t, n, periods, n_periods, widths, prow.data(), cost, uniform, M, flux_sigma, y_abs_max, params->transit_depth_min, ctx->opt, order);

    // launch geometry, and the device buffers it asks for
    if (const char* why = plan_search(ctx->plan, n, widths, uniform, n_periods, ctx->n_cu, ctx->opt, prow.data(), order.data()))
        return fail(ctx, TLS_E_ARG, why);
    { int rcb = reserve_plan_buffers(ctx); if (rcb) return rcb; }

    ctx->w0 = w0; ctx->S0 = S0; ctx->depth_min = params->transit_depth_min;
    ctx->host_widths = widths;
    ctx->band_sigma = -1.0; ctx->d_band_now = nullptr;   // (d_band belongs to the previous width table)
    choose_flux_kernels(ctx, flux_sigma);
    ctx->plan_counters = tls_counters{gp.cells, 0, 0, gp.pairs, 0};

    { int rcs = stage_plan(ctx, t, y, w, periods, order, prow, widths, q); if (rcs) return rcs; }
    key_store(ctx->key, ctx->opt, t, n, periods, n_periods, tmpl, params);
    ctx->prepared = true;
    return TLS_OK;
}

namespace {
// A plain search of the held plan and flux may overlap its neighbours: lanes on, the four-slot kernel, one light curve from
// the context's own buffers, and a table of folded orders that is filled (such a launch writes nothing but its lane's state).
bool launch_overlappable(const tls_ctx* ctx) {
    return ctx->lanes != 0 && ctx->perm_table_entries > 0 && ctx->perm_filled && ctx->batch_curves == 1 && !ctx->over_y &&
           !ctx->over_w && !ctx->over_S0 && !ctx->over_w0 && !ctx->over_chi2 && !ctx->over_row && !ctx->over_depth &&
           is_slim(pick_kernel(ctx->plan, ctx->flux));
}

// the flux of the next search into lane B's buffer, on lane B's stream (behind lane B's earlier launch, and nothing newer)
int update_flux_lane_b(tls_ctx* ctx, const double* y) {
    auto& lb = ctx->lane_b;
    const size_t bytes = (size_t)ctx->plan.n * 8;
    if (int rc = ensure_lane_b(ctx)) return rc;
    if (lb.stage_pending) { TLS_HIP(ctx, hipEventSynchronize(lb.ev_stage)); lb.stage_pending = false; }
    if (lb.h_stage_cap < bytes) {
        if (lb.h_stage) TLS_HIP(ctx, hipHostFree(lb.h_stage));
        lb.h_stage = nullptr; lb.h_stage_cap = 0;
        const size_t cap = std::max<size_t>(bytes + bytes / 4, 1 << 16);
        TLS_HIP(ctx, hipHostMalloc(reinterpret_cast<void**>(&lb.h_stage), cap, hipHostMallocDefault));
        lb.h_stage_cap = cap;
    }
    std::memcpy(lb.h_stage, y, bytes);
    if (int rc = lane_b_see_state(ctx)) return rc;
    TLS_HIP(ctx, hipMemcpyAsync(lb.d_y.ptr, lb.h_stage, bytes, hipMemcpyHostToDevice, lb.stream));
    TLS_HIP(ctx, hipEventRecord(lb.ev_stage, lb.stream));
    lb.stage_pending = true;
    TLS_HIP(ctx, hipEventRecord(lb.ev_done, lb.stream));
    lb.outstanding = true;
    ctx->flux_b_unseen = true;
    ctx->d_y.ptr = lb.d_y.ptr; ctx->flux_lane = 1;
    return TLS_OK;
}

// ... and into lane A's, on lane A's stream without a join (the launch in flight on lane B reads lane B's flux)
int update_flux_lane_a(tls_ctx* ctx, const double* y) {
    const PlanLayout& L = ctx->layout;
    const size_t bytes = (size_t)ctx->plan.n * 8;
    if (int rc = stage_reserve(ctx, L.total)) return rc;
    std::memcpy(ctx->h_stage + L.y, y, bytes);
    TLS_HIP(ctx, hipMemcpyAsync(ctx->d_y_a.ptr, ctx->h_stage + L.y, bytes, hipMemcpyHostToDevice, ctx->lane_a_stream));
    TLS_HIP(ctx, hipEventRecord(ctx->ev_stage, ctx->lane_a_stream));
    ctx->stage_pending = true;
    ctx->state_dirty = true;   // (lane B's next command has to see this upload)
    ctx->d_y.ptr = ctx->d_y_a.ptr; ctx->flux_lane = 0;
    return TLS_OK;
}

// the flux (and weights) of a prepared plan replaced; kWeightsDiffer when the new dy changes the weight structure
int update_flux_impl(tls_ctx* ctx, const double* y, const double* dy) {
    std::vector<double> w;
    bool uniform; double w0, S0;
    double y_abs_max = 0.0, e_abs_max = 0.0;
    weights_from(y, dy, ctx->plan.n, uniform, w0, w, S0, &y_abs_max, &e_abs_max);
    if (uniform != ctx->plan.uniform) return kWeightsDiffer;
    ctx->w0 = w0; ctx->S0 = S0; ctx->y_abs_max = y_abs_max; ctx->e_abs_max = e_abs_max;
    choose_flux_kernels(ctx, flux_scatter(y, ctx->plan.n));
    const PlanLayout& L = ctx->layout;
    const size_t nn = (size_t)ctx->plan.n;
    // Inside a run of overlappable searches the flux goes to the lane the NEXT search takes, on that lane's stream: it waits
    // for that lane's earlier launch through stream order and for nothing else -- the launch in flight on the other lane
    // keeps reading its own flux.  (S0, w0, y_abs_max and the kernel choice are kernel arguments, taken at enqueue.)
    if (ctx->run_lane >= 0 && launch_overlappable(ctx)) {
        const int target = ctx->run_lane ^ 1;
        if (target == 1 ? !ctx->a_reads_flux_b : !ctx->b_reads_flux_a) {
            ctx->executed = false;
            return target == 1 ? update_flux_lane_b(ctx, y) : update_flux_lane_a(ctx, y);
        }
    }
    int rcs = stage_reserve(ctx, L.total);   // (waits for the previous upload out of the staging buffer)
    if (rcs) return rcs;
    std::memcpy(ctx->h_stage + L.y, y, nn * 8);
    ctx->d_y.ptr = ctx->d_y_a.ptr; ctx->flux_lane = 0;
    TLS_HIP(ctx, hipMemcpyAsync(ctx->d_y.ptr, ctx->h_stage + L.y, nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    if (!uniform) {
        std::memcpy(ctx->h_stage + L.w, w.data(), nn * 8);
        TLS_HIP(ctx, hipMemcpyAsync(ctx->d_w.ptr, ctx->h_stage + L.w, nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    }
    TLS_HIP(ctx, hipEventRecord(ctx->ev_stage, main_stream(ctx)));
    ctx->stage_pending = true;
    ctx->executed = false;
    return TLS_OK;
}
}  // namespace

int tls_update_flux(tls_ctx* ctx, const double* y, const double* dy) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (!ctx->prepared) return fail(ctx, TLS_E_STATE, "tls_update_flux before tls_prepare");
    if (!y || !dy) return fail(ctx, TLS_E_ARG, "null argument");
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    const int rc = update_flux_impl(ctx, y, dy);
    if (rc == kWeightsDiffer)
        return fail(ctx, TLS_E_STATE, "weight structure (uniform / per-point dy) differs from the prepared search");
    return rc;
}

int tls_execute(tls_ctx* ctx, int count_work) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (!ctx->prepared) return fail(ctx, TLS_E_STATE, "tls_execute before tls_prepare");
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->plan.n_periods == 0) { ctx->executed = true; return TLS_OK; }
    // Launch lanes: a plain four-slot search whose table of folded orders was filled before the PREVIOUS launch was enqueued
    // (so that lane A's recorded state covers the filling launch) may overlap its neighbours.  It takes lane B when the launch
    // before it was such a one on lane A and nothing but tls_update_flux came between; otherwise lane A.  Every other launch
    // joins the lanes and runs on lane A as ever.
    int lane = -1;
    if (count_work == 0 && ctx->perm_filled_before_prev && launch_overlappable(ctx)) lane = ctx->run_lane == 0 ? 1 : 0;
    return enqueue(ctx, (count_work & 1) != 0, (count_work & 2) != 0, nullptr, nullptr, nullptr, lane);
}

int tls_t0_fit(tls_ctx* ctx, const double* t, const double* y, int64_t n, double period, const double* signal,
               int64_t dur, const double* epochs, int64_t n_epochs, int64_t roll, double* out_residuals) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (!t || !y || !signal || !epochs || !out_residuals) return fail(ctx, TLS_E_ARG, "null argument");
    if (n < 3 || n > 50000000 || dur < 1 || dur > n || n_epochs < 0 || roll < 0 || !(period > 0))
        return fail(ctx, TLS_E_ARG, "tls_t0_fit: argument out of range");
    if (n_epochs == 0) return TLS_OK;
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    TLS_HIP(ctx, ctx->d_queue.reserve(1));
    int rc;
    if ((rc = upload(ctx, ctx->d_ft, t, (size_t)n))) return rc;
    if ((rc = upload(ctx, ctx->d_fy, y, (size_t)n))) return rc;
    if ((rc = upload(ctx, ctx->d_fsig, signal, (size_t)dur))) return rc;
    if ((rc = upload(ctx, ctx->d_fep, epochs, (size_t)n_epochs))) return rc;
    TLS_HIP(ctx, ctx->d_fres.reserve((size_t)n_epochs));
    TLS_HIP(ctx, hipMemsetAsync(ctx->d_queue.ptr, 0, sizeof(unsigned int), main_stream(ctx)));
    double t_lo, t_hi;
    time_range(t, n, t_lo, t_hi);
    if ((rc = launch_t0_fit(ctx, ctx->d_ft.ptr, ctx->d_fy.ptr, ctx->d_fsig.ptr, ctx->d_fep.ptr, ctx->d_fres.ptr, ctx->d_queue.ptr,
                            n, period, dur, n_epochs, roll, t_lo, t_hi))) return rc;
    TLS_HIP(ctx, hipMemcpyAsync(out_residuals, ctx->d_fres.ptr, (size_t)n_epochs * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
    TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));
    return TLS_OK;
}

int tls_pink_noise(tls_ctx* ctx, const double* data, int64_t n, int64_t width, double root_width, double* out) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (!data || !out) return fail(ctx, TLS_E_ARG, "null argument");
    if (n < 1 || n > 100000000 || width < 1 || width > n) return fail(ctx, TLS_E_ARG, "pink noise: 1 <= width <= n wanted");
    if (!(root_width > 0.0)) return fail(ctx, TLS_E_ARG, "pink noise: root_width must be width ** 0.5");
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t n_windows = n - width + 1;
    double *d_data, *d_terms, *d_sums;
    Arena L;
    L.add(d_data, (size_t)n);  L.add(d_terms, (size_t)n_windows);  L.add(d_sums, (size_t)n_windows + 1);   // running sums
    TLS_HIP(ctx, L.bind(ctx->d_pink));
    TLS_HIP(ctx, hipMemcpyAsync(d_data, data, (size_t)n * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    hipLaunchKernelGGL(tlsdev::tls_pink_terms, dim3((unsigned)((n_windows + 255) / 256)), dim3(256), 0, main_stream(ctx),
                       (const double*)d_data, (int)n_windows, (int)width, root_width, d_terms);
    TLS_HIP(ctx, hipGetLastError());
    // (the reference adds the terms one by one from the left: the exact sequential prefix sum of the search, terms >= 0)
    hipLaunchKernelGGL(tlsdev::tls_cumsum_kernel, dim3(1), dim3(1024), 0, main_stream(ctx), (const double*)d_terms, d_sums, (int)n_windows, 0,
                       static_cast<unsigned long long*>(nullptr));
    TLS_HIP(ctx, hipGetLastError());
    double last = 0.0;
    TLS_HIP(ctx, hipMemcpyAsync(&last, d_sums + n_windows, 8, hipMemcpyDeviceToHost, main_stream(ctx)));
    TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));
    *out = last / (double)n_windows;
    return TLS_OK;
}

static_assert(sizeof(tls_injection) == 6 * sizeof(double), "tls_injection is six doubles");

int tls_inject_transits(tls_ctx* ctx, const double* t, int64_t n, const double* flux, int64_t flux_rows,
                        const tls_injection* inj, int64_t n_inj, double u1, double u2, double* out_flux,
                        int64_t* out_in_transit) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (n < 1 || n > 100000000) return fail(ctx, TLS_E_ARG, "inject: n out of range [1, 1e8]");
    if (n_inj < 0) return fail(ctx, TLS_E_ARG, "inject: n_inj < 0");
    if (n_inj == 0) return TLS_OK;
    if (flux_rows != 1 && flux_rows != n_inj) return fail(ctx, TLS_E_ARG, "inject: flux_rows must be 1 or n_inj");
    if (!t || !flux || !inj || !out_flux) return fail(ctx, TLS_E_ARG, "null argument");
    if (!std::isfinite(u1) || !std::isfinite(u2)) return fail(ctx, TLS_E_ARG, "inject: non-finite limb darkening");
    for (int64_t k = 0; k < n_inj; ++k) {
        const tls_injection& c = inj[k];
        if (!std::isfinite(c.tp) || !std::isfinite(c.period) || !std::isfinite(c.rp) || !std::isfinite(c.a)
            || !std::isfinite(c.sin_inc) || !std::isfinite(c.omega))
            return fail(ctx, TLS_E_ARG, "inject: injection " + std::to_string(k) + " has a non-finite constant");
        if (!(c.period > 0.0) || !(c.a > 0.0) || !(c.rp >= 0.0))
            return fail(ctx, TLS_E_ARG, "inject: injection " + std::to_string(k) + " needs period > 0, a > 0 and rp >= 0");
    }
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    // rows per launch: the slab's injected rows stay within 256 MB (and gridDim.y within its limit)
    const size_t nn = (size_t)n;
    const int64_t slab = std::max<int64_t>(1, std::min<int64_t>({n_inj, (int64_t)65535, (int64_t)((256u << 20) / (8 * nn))}));
    const size_t base_len = flux_rows == 1 ? nn : (size_t)slab * nn;
    double *d_t, *d_base, *d_out, *d_consts;
    Arena L;
    L.add(d_t, nn);  L.add(d_base, base_len);  L.add(d_out, (size_t)slab * nn);   // the injected rows of one slab
    L.add(d_consts, 6 * (size_t)slab);   // ... and their constants (tls_injection)
    TLS_HIP(ctx, L.bind(ctx->d_inject));
    TLS_HIP(ctx, ctx->d_inject_count.reserve((size_t)slab));
    TLS_HIP(ctx, hipMemcpyAsync(d_t, t, nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    if (flux_rows == 1) TLS_HIP(ctx, hipMemcpyAsync(d_base, flux, nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    for (int64_t k0 = 0; k0 < n_inj; k0 += slab) {
        const int64_t rows = std::min<int64_t>(slab, n_inj - k0);
        if (flux_rows != 1)
            TLS_HIP(ctx, hipMemcpyAsync(d_base, flux + (size_t)k0 * nn, (size_t)rows * nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
        TLS_HIP(ctx, hipMemcpyAsync(d_consts, inj + k0, (size_t)rows * sizeof(tls_injection), hipMemcpyHostToDevice, main_stream(ctx)));
        TLS_HIP(ctx, hipMemsetAsync(ctx->d_inject_count.ptr, 0, (size_t)rows * sizeof(unsigned long long), main_stream(ctx)));
        tlsdev::InjectArgs a;
        a.t = d_t; a.flux = d_base; a.consts = d_consts; a.u1 = u1; a.u2 = u2; a.out = d_out;
        a.count = ctx->d_inject_count.ptr; a.n = (long long)n; a.flux_stride = flux_rows == 1 ? 0 : (long long)n;
        hipLaunchKernelGGL(tlsdev::tls_inject_transits, dim3((unsigned)((n + 255) / 256), (unsigned)rows), dim3(256), 0,
                           main_stream(ctx), a);
        TLS_HIP(ctx, hipGetLastError());
        ctx->last_kernel = "tls_inject_transits";
        TLS_HIP(ctx, hipMemcpyAsync(out_flux + (size_t)k0 * nn, d_out, (size_t)rows * nn * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        if (out_in_transit) {
            static_assert(sizeof(unsigned long long) == sizeof(int64_t), "count width");
            TLS_HIP(ctx, hipMemcpyAsync(out_in_transit + k0, ctx->d_inject_count.ptr, (size_t)rows * 8, hipMemcpyDeviceToHost,
                                        main_stream(ctx)));
        }
        // (the next slab overwrites the device rows: the copies above have to be done first)
        TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));
    }
    return TLS_OK;
}

// Checks shared by tls_null_rows and tls_debug_null_words; *blocks = Philox blocks per trial (W / 4).
static int null_check(tls_ctx* ctx, int64_t n, int64_t n_rows, int64_t first_trial, int mode, int64_t block, int64_t* blocks) {
    if (n < 1 || n > 100000000) return fail(ctx, TLS_E_ARG, "null rows: n out of range [1, 1e8]");
    if (n_rows < 0) return fail(ctx, TLS_E_ARG, "null rows: n_rows < 0");
    if (first_trial < 0) return fail(ctx, TLS_E_ARG, "null rows: first_trial < 0");
    int64_t words;
    if (mode == 0) {
        words = 2 * n;
    } else if (mode == 1) {
        if (block < 1 || block > n) return fail(ctx, TLS_E_ARG, "null rows: block out of range [1, n]");
        words = (n + block - 1) / block;
    } else {
        return fail(ctx, TLS_E_ARG, "null rows: mode must be 0 (white noise) or 1 (block bootstrap)");
    }
    *blocks = (words + 3) / 4;
    // the last block's counter, (first_trial + n_rows) W / 4, must stay below 2^64 (counter words 1..3 stay 0)
    if (first_trial > INT64_MAX - n_rows || (uint64_t)(first_trial + n_rows) > (UINT64_MAX - 1) / (uint64_t)*blocks)
        return fail(ctx, TLS_E_ARG, "null rows: trial indices past the 64-bit Philox counter");
    return TLS_OK;
}

// rows per launch: at most 256 MB of rows, and gridDim.y within its limit
static int64_t null_slab(int64_t n_rows, size_t row_bytes) {
    return std::max<int64_t>(1, std::min<int64_t>({n_rows, (int64_t)65535, (int64_t)((256u << 20) / row_bytes)}));
}

int tls_null_rows(tls_ctx* ctx, int64_t n, int64_t n_rows, uint64_t seed, int64_t first_trial, int mode,
                  const double* sigma, int64_t n_sigma, const double* src, int64_t n_src, int64_t block, double* out) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    int64_t blocks = 0;
    if (int rc = null_check(ctx, n, n_rows, first_trial, mode, block, &blocks)) return rc;
    if (mode == 0) {
        if (n_sigma != 1 && n_sigma != n_rows) return fail(ctx, TLS_E_ARG, "null rows: n_sigma must be 1 or n_rows");
        if (!sigma) return fail(ctx, TLS_E_ARG, "null argument");
        for (int64_t k = 0; k < n_sigma; ++k)
            if (!(sigma[k] > 0.0 && sigma[k] <= 0.1))
                return fail(ctx, TLS_E_ARG, "null rows: sigma " + std::to_string(k) + " outside (0, 0.1]");
    } else {
        if (n_src < 1) return fail(ctx, TLS_E_ARG, "null rows: n_src < 1");
        if (!src) return fail(ctx, TLS_E_ARG, "null argument");
        if ((uint64_t)n_src > (uint64_t)(SIZE_MAX / 8) / (uint64_t)n) return fail(ctx, TLS_E_ARG, "null rows: source too large");
        for (size_t k = 0; k < (size_t)n_src * (size_t)n; ++k)
            if (!(std::isfinite(src[k]) && src[k] > 0.0))
                return fail(ctx, TLS_E_ARG, "null rows: source row " + std::to_string(k / (size_t)n)
                                            + " has a non-finite or non-positive value");
    }
    if (n_rows == 0) return TLS_OK;
    if (!out) return fail(ctx, TLS_E_ARG, "null argument");
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)n;
    const int64_t slab = null_slab(n_rows, 8 * nn);
    const size_t src_len = mode == 1 ? (size_t)n_src * nn : 0;
    const size_t sigma_len = mode == 0 ? (size_t)n_sigma : 0;
    double *d_src, *d_sigma, *d_out;
    Arena L;
    L.add(d_src, src_len);  L.add(d_sigma, sigma_len);  L.add(d_out, (size_t)slab * nn);   // the rows of one slab
    TLS_HIP(ctx, L.bind(ctx->d_null));
    if (src_len) TLS_HIP(ctx, hipMemcpyAsync(d_src, src, src_len * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    if (sigma_len) TLS_HIP(ctx, hipMemcpyAsync(d_sigma, sigma, sigma_len * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    for (int64_t k0 = 0; k0 < n_rows; k0 += slab) {
        const int64_t rows = std::min<int64_t>(slab, n_rows - k0);
        tlsdev::NullArgs a;
        a.out = d_out; a.src = d_src; a.seed = (unsigned long long)seed; a.first_trial = (long long)(first_trial + k0);
        a.blocks = (long long)blocks; a.n_src = (long long)n_src; a.n = (unsigned int)n; a.L = (unsigned int)block;
        a.sigma_stride = n_sigma == 1 ? 0 : 1;
        a.sigma = mode == 0 ? d_sigma + (n_sigma == 1 ? 0 : k0) : nullptr;
        if (mode == 0) {
            hipLaunchKernelGGL(tlsdev::tls_null_white, dim3((unsigned)((blocks + 255) / 256), (unsigned)rows), dim3(256), 0,
                               main_stream(ctx), a);
            ctx->last_kernel = "tls_null_white";
        } else {
            hipLaunchKernelGGL(tlsdev::tls_null_bootstrap, dim3((unsigned)((n + 255) / 256), (unsigned)rows), dim3(256), 0,
                               main_stream(ctx), a);
            ctx->last_kernel = "tls_null_bootstrap";
        }
        TLS_HIP(ctx, hipGetLastError());
        TLS_HIP(ctx, hipMemcpyAsync(out + (size_t)k0 * nn, d_out, (size_t)rows * nn * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        // (the next slab overwrites the device rows: the copy above has to be done first)
        TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));
    }
    return TLS_OK;
}

int tls_debug_null_words(tls_ctx* ctx, int64_t n, int64_t n_rows, uint64_t seed, int64_t first_trial, int mode,
                         int64_t block, uint64_t* out) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    int64_t blocks = 0;
    if (int rc = null_check(ctx, n, n_rows, first_trial, mode, block, &blocks)) return rc;
    if (n_rows == 0) return TLS_OK;
    if (!out) return fail(ctx, TLS_E_ARG, "null argument");
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t W = 4 * (size_t)blocks;
    const int64_t slab = null_slab(n_rows, 8 * W);
    TLS_HIP(ctx, ctx->d_null_words.reserve((size_t)slab * W));
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "word width");
    for (int64_t k0 = 0; k0 < n_rows; k0 += slab) {
        const int64_t rows = std::min<int64_t>(slab, n_rows - k0);
        tlsdev::NullArgs a{};
        a.seed = (unsigned long long)seed; a.first_trial = (long long)(first_trial + k0); a.blocks = (long long)blocks;
        hipLaunchKernelGGL(tlsdev::tls_null_words, dim3((unsigned)((blocks + 255) / 256), (unsigned)rows), dim3(256), 0,
                           main_stream(ctx), a, ctx->d_null_words.ptr);
        TLS_HIP(ctx, hipGetLastError());
        ctx->last_kernel = "tls_null_words";
        TLS_HIP(ctx, hipMemcpyAsync(out + (size_t)k0 * W, ctx->d_null_words.ptr, (size_t)rows * W * 8, hipMemcpyDeviceToHost,
                                    main_stream(ctx)));
        TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));
    }
    return TLS_OK;
}

static_assert(TLS_MEDFILT_MAX_KERNEL - 1 <= tlsdev::kDetrendMaxSpan / 2, "the largest kernel's span fits kDetrendMaxSpan");

// P (sorted slots, a power of two) of a tile of tls_medfilt_detrend: about 2 (k - 1), so that a tile has as many outputs
// as halo slots, at least 256 (no fewer than 128 outputs a tile), and no more than the whole row's span needs (small n).
static int detrend_span(int64_t n, int64_t k) {
    auto pow2 = [](int64_t v) { int64_t p = 64; while (p < v) p <<= 1; return (int)p; };
    return std::min(pow2(std::max<int64_t>(2 * (k - 1), 256)), pow2(n + k - 1));
}

int tls_medfilt_detrend(tls_ctx* ctx, const double* y, int64_t n, int64_t n_rows, int64_t kernel, double* out_flat,
                        double* out_trend) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (n < 1 || n > 100000000) return fail(ctx, TLS_E_ARG, "medfilt: n out of range [1, 1e8]");
    if (n_rows < 0) return fail(ctx, TLS_E_ARG, "medfilt: n_rows < 0");
    if (kernel < 1 || kernel % 2 == 0) return fail(ctx, TLS_E_ARG, "medfilt: the kernel size must be odd and >= 1");
    if (kernel > n) return fail(ctx, TLS_E_ARG, "medfilt: the kernel size exceeds the row length n");
    if (kernel > TLS_MEDFILT_MAX_KERNEL)
        return fail(ctx, TLS_E_ARG, "medfilt: the kernel size exceeds " + std::to_string(TLS_MEDFILT_MAX_KERNEL));
    if (n_rows == 0) return TLS_OK;
    if (!y || !out_flat) return fail(ctx, TLS_E_ARG, "null argument");
    if ((uint64_t)n_rows > (uint64_t)(SIZE_MAX / 8) / (uint64_t)n) return fail(ctx, TLS_E_ARG, "medfilt: rows too large");
    const size_t nn = (size_t)n;
    for (size_t q = 0; q < (size_t)n_rows * nn; ++q)
        if (!(std::isfinite(y[q]) && y[q] > 0.0))
            return fail(ctx, TLS_E_ARG, "medfilt: row " + std::to_string(q / nn) + " has a non-finite or non-positive value");
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    // rows per launch: at most 256 MB of rows (as the injection and null slabs), and gridDim.y within its limit
    const int64_t slab = std::max<int64_t>(1, std::min<int64_t>({n_rows, (int64_t)65535, (int64_t)((256u << 20) / (8 * nn))}));
    double *d_y, *d_flat, *d_trend;
    Arena L;
    L.add(d_y, (size_t)slab * nn);  L.add(d_flat, (size_t)slab * nn);  L.add(d_trend, out_trend ? (size_t)slab * nn : 0);
    TLS_HIP(ctx, L.bind(ctx->d_detrend));
    const int P = detrend_span(n, kernel);
    const int T = P - (int)(kernel - 1);
    const size_t lds = (size_t)P * (sizeof(unsigned long long) + sizeof(unsigned int));
    auto fn = tlsdev::tls_medfilt_detrend;
    TLS_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    tlsdev::DetrendArgs a;
    a.y = d_y; a.flat = d_flat; a.trend = d_trend; a.check = nullptr;
    a.n = (long long)n; a.k = (int)kernel; a.span = P; a.tile = T;
#ifdef TLS_DEBUG_CHECKS
    if (int rc = ensure_check_counters(ctx)) return rc;
    a.check = ctx->d_check.ptr;
#endif
    const unsigned tiles = (unsigned)((n + T - 1) / T);
    for (int64_t k0 = 0; k0 < n_rows; k0 += slab) {
        const int64_t rows = std::min<int64_t>(slab, n_rows - k0);
        const size_t bytes = (size_t)rows * nn * 8;
        TLS_HIP(ctx, hipMemcpyAsync(d_y, y + (size_t)k0 * nn, bytes, hipMemcpyHostToDevice, main_stream(ctx)));
        hipLaunchKernelGGL(fn, dim3(tiles, (unsigned)rows), dim3(tlsdev::kDetrendThreads), lds, main_stream(ctx), a);
        TLS_HIP(ctx, hipGetLastError());
        ctx->last_kernel = "tls_medfilt_detrend";
        TLS_HIP(ctx, hipMemcpyAsync(out_flat + (size_t)k0 * nn, d_flat, bytes, hipMemcpyDeviceToHost, main_stream(ctx)));
        if (out_trend)
            TLS_HIP(ctx, hipMemcpyAsync(out_trend + (size_t)k0 * nn, d_trend, bytes, hipMemcpyDeviceToHost, main_stream(ctx)));
        // (the next slab overwrites the device rows: the copies above have to be done first)
        TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));
    }
    return TLS_OK;
}

static_assert(2 * (TLS_BIWEIGHT_MAX_WINDOW - 1) + 4 <= tlsdev::kDetrendMaxSpan, "a tile at the largest window holds 4 outputs");
static_assert(12 * tlsdev::kDetrendMaxSpan + 8 * tlsdev::kDetrendMaxSpan <= 160 * 1024, "the largest span fits the LDS");

// The tiles of tls_biweight_detrend, from the windows [lo_i, hi_i) of the call (at most wmax points each).  P0 = about
// 4 (wmax - 1), at least 256 and at most kDetrendMaxSpan; a row of n <= P0 points is one tile, otherwise a tile has
// T = P0 - 2 (wmax - 1) outputs, so that its span [lo_first, hi_last) holds at most T + 2 (wmax - 1) = P0 slots (lo_i >=
// i - (wmax - 1), hi_i <= i + wmax).  smax is the largest span of the call's tiles and P the power of two (>= 64) that sorts it.
static void biweight_plan(const std::vector<int>& lo, const std::vector<int>& hi, int64_t wmax, int* T, int* P, int* smax) {
    auto pow2 = [](int64_t v) { int64_t p = 64; while (p < v) p <<= 1; return (int)p; };
    const int64_t n = (int64_t)lo.size();
    const int64_t P0 = std::min<int64_t>(pow2(std::max<int64_t>(4 * (wmax - 1), 256)), tlsdev::kDetrendMaxSpan);
    const int64_t tile = n <= P0 ? n : P0 - 2 * (wmax - 1);
    int64_t s = 1;
    for (int64_t f = 0; f < n; f += tile) s = std::max<int64_t>(s, hi[std::min(f + tile, n) - 1] - lo[f]);
    *T = (int)tile;
    *smax = (int)s;
    *P = pow2(s);
}

// tls_biweight_detrend (masked false: mask, min_points and out_status are not looked at) and tls_biweight_detrend_masked
static int biweight_detrend(tls_ctx* ctx, const double* t, const double* y, bool masked, const uint8_t* mask, int64_t n,
                            int64_t n_rows, double window_length, double break_tolerance, int64_t min_points, double* out_flat,
                            double* out_trend, uint8_t* out_status) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (n < 1 || n > 100000000) return fail(ctx, TLS_E_ARG, "biweight: n out of range [1, 1e8]");
    if (n_rows < 0) return fail(ctx, TLS_E_ARG, "biweight: n_rows < 0");
    if (masked && (min_points < 1 || min_points > INT32_MAX)) return fail(ctx, TLS_E_ARG, "biweight: min_points must be >= 1");
    if (!(std::isfinite(window_length) && window_length > 0.0))
        return fail(ctx, TLS_E_ARG, "biweight: window_length must be finite and > 0");
    if (!(break_tolerance > 0.0)) return fail(ctx, TLS_E_ARG, "biweight: break_tolerance must be > 0");
    if (!t) return fail(ctx, TLS_E_ARG, "null argument");
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(t[i]) || (i > 0 && !(t[i] >= t[i - 1])))
            return fail(ctx, TLS_E_ARG, "biweight: t must be finite and non-decreasing (index " + std::to_string(i) + ")");
    // the windows: [lo_i, hi_i) inside i's segment, |t[j] - t[i]| <= window_length / 2 (both ends only move forward)
    std::vector<int> lo((size_t)n), hi((size_t)n);
    const double half = 0.5 * window_length;
    int64_t seg = 0, wlo = 0, whi = 0, wmax = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (i > 0 && t[i] - t[i - 1] > break_tolerance) seg = i;
        wlo = std::max(wlo, seg);
        while (std::fabs(t[wlo] - t[i]) > half) ++wlo;
        whi = std::max(whi, i + 1);
        while (whi < n && !(t[whi] - t[whi - 1] > break_tolerance) && std::fabs(t[whi] - t[i]) <= half) ++whi;
        lo[(size_t)i] = (int)wlo;
        hi[(size_t)i] = (int)whi;
        wmax = std::max(wmax, whi - wlo);
    }
    if (wmax > TLS_BIWEIGHT_MAX_WINDOW)
        return fail(ctx, TLS_E_ARG, "biweight: a window holds " + std::to_string(wmax) + " points, more than " +
                                        std::to_string(TLS_BIWEIGHT_MAX_WINDOW));
    if (n_rows == 0) return TLS_OK;
    if (!y || !out_flat || (masked && !mask)) return fail(ctx, TLS_E_ARG, "null argument");
    if ((uint64_t)n_rows > (uint64_t)(SIZE_MAX / 8) / (uint64_t)n) return fail(ctx, TLS_E_ARG, "biweight: rows too large");
    const size_t nn = (size_t)n;
    for (size_t q = 0; q < (size_t)n_rows * nn; ++q)
        if (!(std::isfinite(y[q]) && y[q] > 0.0))
            return fail(ctx, TLS_E_ARG, "biweight: row " + std::to_string(q / nn) + " has a non-finite or non-positive value");
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    // rows per launch: at most 256 MB of rows (as the median filter's slabs), and gridDim.y within its limit
    const int64_t slab = std::max<int64_t>(1, std::min<int64_t>({n_rows, (int64_t)65535, (int64_t)((256u << 20) / (8 * nn))}));
    double *d_y, *d_flat, *d_trend;
    Arena L;
    L.add(d_y, (size_t)slab * nn);  L.add(d_flat, (size_t)slab * nn);
    L.add(d_trend, out_trend || masked ? (size_t)slab * nn : 0);   // (the masked call interpolates between trend values: it always forms them)
    TLS_HIP(ctx, L.bind(ctx->d_detrend));
    int *d_lo, *d_hi;   // the window of every point
    Arena W;
    W.add(d_lo, nn);  W.add(d_hi, nn);
    TLS_HIP(ctx, W.bind(ctx->d_windows));
    // the masked call: the time stamps; the mask rows, the masked pass's marks and the status rows of a slab
    unsigned char *d_mask = nullptr, *d_open = nullptr, *d_status = nullptr;
    if (masked) {
        TLS_HIP(ctx, ctx->d_protect.reserve(nn));
        Arena M;
        M.add(d_mask, (size_t)slab * nn);  M.add(d_open, (size_t)slab * nn);  M.add(d_status, (size_t)slab * nn);
        TLS_HIP(ctx, M.bind(ctx->d_protect_bytes));
        TLS_HIP(ctx, hipMemcpyAsync(ctx->d_protect.ptr, t, nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    }
    TLS_HIP(ctx, hipMemcpyAsync(d_lo, lo.data(), nn * sizeof(int), hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_hi, hi.data(), nn * sizeof(int), hipMemcpyHostToDevice, main_stream(ctx)));
    int T = 0, P = 0, smax = 0;
    biweight_plan(lo, hi, wmax, &T, &P, &smax);
    const size_t lds = (size_t)P * (sizeof(unsigned long long) + sizeof(unsigned int)) + (size_t)smax * sizeof(double);
    auto fn = tlsdev::tls_biweight_detrend;
    auto fn_masked = tlsdev::tls_biweight_detrend_masked;
    auto fn_fallback = tlsdev::tls_biweight_detrend_fallback;
    if (masked) {
        TLS_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(fn_masked), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        TLS_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(fn_fallback), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    } else {
        TLS_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    tlsdev::BiweightMaskedArgs a;   // (the plain kernel takes its base, BiweightArgs)
    a.mask = d_mask; a.status = d_open; a.min_points = (int)min_points;
    a.y = d_y; a.flat = d_flat; a.trend = d_trend; a.check = nullptr;
    a.lo = d_lo; a.hi = d_hi;
    a.n = (long long)n; a.tile = T; a.span = P; a.smax = smax;
#ifdef TLS_DEBUG_CHECKS
    if (int rc = ensure_check_counters(ctx)) return rc;
    a.check = ctx->d_check.ptr;
#endif
    const unsigned tiles = (unsigned)((n + T - 1) / T);
    for (int64_t k0 = 0; k0 < n_rows; k0 += slab) {
        const int64_t rows = std::min<int64_t>(slab, n_rows - k0);
        const size_t bytes = (size_t)rows * nn * 8;
        TLS_HIP(ctx, hipMemcpyAsync(d_y, y + (size_t)k0 * nn, bytes, hipMemcpyHostToDevice, main_stream(ctx)));
        if (!masked) {
            hipLaunchKernelGGL(fn, dim3(tiles, (unsigned)rows), dim3(tlsdev::kDetrendThreads), lds, main_stream(ctx),
                               static_cast<const tlsdev::BiweightArgs&>(a));
            TLS_HIP(ctx, hipGetLastError());
            ctx->last_kernel = "tls_biweight_detrend";
        } else {
            // the members' biweight where a window holds min_points of them; the open points from their neighbours; the plain
            // biweight where a whole segment is open
            TLS_HIP(ctx, hipMemcpyAsync(d_mask, mask + (size_t)k0 * nn, (size_t)rows * nn, hipMemcpyHostToDevice, main_stream(ctx)));
            a.status = d_open;
            hipLaunchKernelGGL(fn_masked, dim3(tiles, (unsigned)rows), dim3(tlsdev::kDetrendThreads), lds, main_stream(ctx), a);
            TLS_HIP(ctx, hipGetLastError());
            tlsdev::BiweightFillArgs f;
            f.t = ctx->d_protect.ptr; f.y = d_y; f.flat = d_flat; f.trend = d_trend; f.open = d_open; f.status = d_status;
            f.n = (long long)n; f.count = (long long)rows * (long long)n; f.break_tolerance = break_tolerance;
            const unsigned blocks = (unsigned)std::min<long long>((f.count + tlsdev::kDetrendThreads - 1) / tlsdev::kDetrendThreads, 65536);
            hipLaunchKernelGGL(tlsdev::tls_biweight_fill, dim3(blocks), dim3(tlsdev::kDetrendThreads), 0, main_stream(ctx), f);
            TLS_HIP(ctx, hipGetLastError());
            a.status = d_status;
            hipLaunchKernelGGL(fn_fallback, dim3(tiles, (unsigned)rows), dim3(tlsdev::kDetrendThreads), lds, main_stream(ctx), a);
            TLS_HIP(ctx, hipGetLastError());
            ctx->last_kernel = "tls_biweight_detrend_masked";
            if (out_status)
                TLS_HIP(ctx, hipMemcpyAsync(out_status + (size_t)k0 * nn, d_status, (size_t)rows * nn, hipMemcpyDeviceToHost, main_stream(ctx)));
        }
        TLS_HIP(ctx, hipMemcpyAsync(out_flat + (size_t)k0 * nn, d_flat, bytes, hipMemcpyDeviceToHost, main_stream(ctx)));
        if (out_trend)
            TLS_HIP(ctx, hipMemcpyAsync(out_trend + (size_t)k0 * nn, d_trend, bytes, hipMemcpyDeviceToHost, main_stream(ctx)));
        // (the next slab overwrites the device rows, and lo / hi live on this stack: the copies have to be done first)
        TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));
    }
    return TLS_OK;
}

int tls_biweight_detrend(tls_ctx* ctx, const double* t, const double* y, int64_t n, int64_t n_rows, double window_length,
                         double break_tolerance, double* out_flat, double* out_trend) {
    return biweight_detrend(ctx, t, y, false, nullptr, n, n_rows, window_length, break_tolerance, 1, out_flat, out_trend, nullptr);
}

int tls_biweight_detrend_masked(tls_ctx* ctx, const double* t, const double* y, const uint8_t* mask, int64_t n, int64_t n_rows,
                                double window_length, double break_tolerance, int64_t min_points, double* out_flat,
                                double* out_trend, uint8_t* out_status) {
    return biweight_detrend(ctx, t, y, true, mask, n, n_rows, window_length, break_tolerance, min_points, out_flat, out_trend,
                            out_status);
}

// ---- the in-transit flags of a batch (tls_protect.hip.h)
int tls_transit_mask(tls_ctx* ctx, const double* t, int64_t n, const int64_t* curve, const double* period, const double* T0,
                     const double* duration, int64_t n_candidates, double factor, int64_t n_curves, uint8_t* out_mask) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (n < 1 || n > 100000000) return fail(ctx, TLS_E_ARG, "transit mask: n out of range [1, 1e8]");
    if (n_curves < 0 || n_candidates < 0) return fail(ctx, TLS_E_ARG, "transit mask: n_curves < 0 or n_candidates < 0");
    if (!(std::isfinite(factor) && factor > 0.0)) return fail(ctx, TLS_E_ARG, "transit mask: factor must be finite and > 0");
    if (!t || (n_candidates > 0 && (!period || !T0 || !duration))) return fail(ctx, TLS_E_ARG, "null argument");
    if (!curve && n_candidates > n_curves) return fail(ctx, TLS_E_ARG, "transit mask: curve out of range [0, n_curves)");
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(t[i])) return fail(ctx, TLS_E_ARG, "transit mask: the time stamps must be finite");
    if (int rc = check_curves(ctx, "transit mask", curve, n_candidates, n_curves)) return rc;
    if (n_curves == 0) return TLS_OK;
    if (!out_mask) return fail(ctx, TLS_E_ARG, "null argument");
    if ((uint64_t)n_curves > (uint64_t)(INT64_MAX / 16) / (uint64_t)n) return fail(ctx, TLS_E_ARG, "transit mask: batch too large");
    // the candidates that take part, grouped by curve in their order of appearance (a stable counting sort)
    const size_t nc = (size_t)n_curves, nn = (size_t)n;
    auto takes_part = [&](int64_t k) {
        return std::isfinite(period[k]) && std::isfinite(T0[k]) && std::isfinite(duration[k]) && period[k] > 0.0 && duration[k] > 0.0;
    };
    std::vector<long long> offset(nc + 1, 0);
    for (int64_t k = 0; k < n_candidates; ++k)
        if (takes_part(k)) ++offset[(size_t)(curve ? curve[k] : k) + 1];
    for (size_t c = 0; c < nc; ++c) offset[c + 1] += offset[c];
    const size_t m = (size_t)offset[nc];
    std::vector<double> sorted(3 * m);
    {
        std::vector<long long> at(offset.begin(), offset.end() - 1);
        for (int64_t k = 0; k < n_candidates; ++k) {
            if (!takes_part(k)) continue;
            const size_t q = (size_t)at[(size_t)(curve ? curve[k] : k)]++;
            sorted[q] = period[k]; sorted[m + q] = T0[k]; sorted[2 * m + q] = duration[k];
        }
    }
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    // curves per launch: at most 256 MB of flags
    const size_t slab = std::max<size_t>(1, std::min<size_t>(nc, ((size_t)256 << 20) / nn));
    double *d_t, *d_cand;
    long long* d_offset;
    Arena L;
    L.add(d_t, nn);  L.add(d_cand, 3 * m);   // period | T0 | duration of the candidates grouped by curve
    L.add(d_offset, nc + 1);
    TLS_HIP(ctx, L.bind(ctx->d_protect));
    TLS_HIP(ctx, ctx->d_protect_bytes.reserve(slab * nn));   // the mask rows of one slab
    TLS_HIP(ctx, hipMemcpyAsync(d_t, t, nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    if (m) TLS_HIP(ctx, hipMemcpyAsync(d_cand, sorted.data(), 3 * m * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_offset, offset.data(), (nc + 1) * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    for (size_t c0 = 0; c0 < nc; c0 += slab) {
        const size_t curves = std::min(slab, nc - c0);
        tlsdev::TransitMaskArgs a;
        a.t = d_t; a.period = d_cand; a.T0 = d_cand + m; a.duration = d_cand + 2 * m; a.offset = d_offset + c0;
        a.mask = ctx->d_protect_bytes.ptr; a.n = (long long)n; a.count = (long long)curves * (long long)n; a.factor = factor;
        const unsigned blocks = (unsigned)std::min<long long>((a.count + tlsdev::kProtectThreads - 1) / tlsdev::kProtectThreads, 65536);
        hipLaunchKernelGGL(tlsdev::tls_transit_mask_kernel, dim3(blocks), dim3(tlsdev::kProtectThreads), 0, main_stream(ctx), a);
        TLS_HIP(ctx, hipGetLastError());
        ctx->last_kernel = "tls_transit_mask";
        TLS_HIP(ctx, hipMemcpyAsync(out_mask + c0 * nn, ctx->d_protect_bytes.ptr, curves * nn, hipMemcpyDeviceToHost, main_stream(ctx)));
        // (the next slab overwrites the device rows, and the sorted candidates live on this stack)
        TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));
    }
    return TLS_OK;
}

// ---- the fitted transits of a batch divided out (tls_remove.hip.h, DESIGN.md "Multi-planet search")
static_assert(sizeof(tlsdev::RemoveCandidate) == tlsdev::kRemoveWords * 8, "a grouped candidate is kRemoveWords doubles");

int tls_remove_transits(tls_ctx* ctx, const double* t, const double* y, int64_t n, int64_t n_curves, const int64_t* curve,
                        const double* period, const double* T0, const int64_t* row, const double* amplitude, const double* b,
                        const double* duration, const double* shift, int64_t n_fits, const double* k_rows, const double* profile,
                        int64_t n_k, int64_t M, const double* sub, int64_t n_sub, double* out_rows, double* out_model,
                        double* out_status) {
#pragma clang fp contract(off)
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    const std::string what = "remove transits";
    if (n_fits < 0 || n_curves < 0 || n < 0) return fail(ctx, TLS_E_ARG, what + ": negative count");
    if (n_k < 1) return fail(ctx, TLS_E_ARG, what + ": every table needs an entry");
    if (n_k > TLS_TRANSIT_FIT_MAX_ROWS) return fail(ctx, TLS_E_ARG, what + ": more than 4096 profile rows");
    if (M < 1 || M > TLS_TRANSIT_FIT_MAX_M) return fail(ctx, TLS_E_ARG, what + ": M out of range [1, 4096]");
    if (n_sub < 1 || n_sub > TLS_TRANSIT_FIT_MAX_SUB) return fail(ctx, TLS_E_ARG, what + ": n_sub out of range [1, 16]");
    if (!k_rows || !profile || !sub) return fail(ctx, TLS_E_ARG, what + ": null argument");
    for (int64_t i = 0; i < n_k; ++i)
        if (!std::isfinite(k_rows[i]) || (i > 0 && k_rows[i] < k_rows[i - 1]))
            return fail(ctx, TLS_E_ARG, what + ": the tables must be finite and non-decreasing");
    if (!(k_rows[0] > 0.0)) return fail(ctx, TLS_E_ARG, what + ": every k_rows must be > 0");
    for (int64_t s = 0; s < n_sub; ++s)
        if (!std::isfinite(sub[s])) return fail(ctx, TLS_E_ARG, what + ": sub must be finite");
    for (int64_t i = 0; i < n_k * (M + 1); ++i)
        if (!std::isfinite(profile[i])) return fail(ctx, TLS_E_ARG, what + ": the profile must be finite");
    if (n_fits > 0 && (!period || !T0 || !row || !amplitude || !b || !duration || !shift || !out_status))
        return fail(ctx, TLS_E_ARG, what + ": null argument");
    if (n_curves > 0 && (!t || !y || !out_rows)) return fail(ctx, TLS_E_ARG, what + ": null argument");
    int rc;
    if (n_curves > 0 || n_fits > 0) {
        if ((rc = check_batch(ctx, what, n, 100000000, "[1, 1e8]", n_fits, n_curves))) return rc;
        if (n_curves > 0 && (rc = check_time_stamps(ctx, what, t, n))) return rc;
    }
    if ((rc = check_curves(ctx, what, curve, n_fits, n_curves, [&](int64_t f) {
            if (row[f] < 0 || row[f] >= n_k) return fail(ctx, TLS_E_ARG, what + ": row out of range [0, n_k)");
            return (int)TLS_OK;
        })))
        return rc;
    if (n_curves == 0) return TLS_OK;
    const size_t nc = (size_t)n_curves, nn = (size_t)n, row_words = (size_t)M + 1;
    // the candidates that take part, with their constants, grouped by curve in their order (a stable counting sort)
    std::vector<tlsdev::RemoveCandidate> made((size_t)n_fits);
    std::vector<long long> offset(nc + 1, 0);
    for (int64_t f = 0; f < n_fits; ++f) {
        const double P = period[f], A = amplitude[f], bf = b[f], T = duration[f];
        const double* p = profile + (size_t)row[f] * row_words;
        double deepest = p[0];
        for (size_t m = 1; m < row_words; ++m) deepest = std::max(deepest, p[m]);
        const double e1 = 1.0 + k_rows[row[f]];
        const double e2 = e1 * e1;
        const double sM = (double)M / e1;
        const double bb = bf * bf;
        const double cc = e2 - bb;
        const double hT = 0.5 * T;
        const double rh = 1.0 / hT;
        const double dip = A * deepest;
        const bool takes_part = std::isfinite(P) && std::isfinite(T0[f]) && std::isfinite(A) && std::isfinite(bf) && std::isfinite(T)
                                && std::isfinite(shift[f]) && P > 0.0 && T > 0.0 && A > 0.0 && bf >= 0.0 && bb < e2 && dip < 1.0;
        out_status[f] = takes_part ? 0.0 : 1.0;
        made[(size_t)f] = tlsdev::RemoveCandidate{P, T0[f], A, shift[f], bb, cc, rh, e2, sM, (double)row[f]};
        if (takes_part) ++offset[(size_t)(curve ? curve[f] : f) + 1];
    }
    for (size_t c = 0; c < nc; ++c) offset[c + 1] += offset[c];
    const size_t m = (size_t)offset[nc];
    if (m == 0) {                                    // nothing to divide out: the rows as they are
        if (out_rows != y) std::memcpy(out_rows, y, nc * nn * 8);
        if (out_model) std::fill(out_model, out_model + nc * nn, 1.0);
        return TLS_OK;
    }
    std::vector<tlsdev::RemoveCandidate> sorted(m);
    {
        std::vector<long long> at(offset.begin(), offset.end() - 1);
        for (int64_t f = 0; f < n_fits; ++f)
            if (out_status[f] == 0.0) sorted[(size_t)at[(size_t)(curve ? curve[f] : f)]++] = made[(size_t)f];
    }
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    // curves per launch: at most 256 MB of rows and models
    const size_t slab = std::max<size_t>(1, std::min<size_t>(nc, ((size_t)256 << 20) / (16 * nn)));
    const size_t table = (size_t)n_k * row_words;
    // all of it written here or by the kernel in front of every read
    double *d_t, *d_profile, *d_sub, *d_rows, *d_model;
    tlsdev::RemoveCandidate* d_cand;
    long long* d_offset;
    Arena L;
    L.add(d_t, nn);  L.add(d_cand, m);   // the grouped candidates
    L.add(d_offset, nc + 1);  L.add(d_profile, table);  L.add(d_sub, (size_t)n_sub);
    L.add(d_rows, slab * nn);    // of one slab: rows | models
    L.add(d_model, slab * nn);
    TLS_HIP(ctx, L.bind(ctx->d_protect));
    if ((rc = ensure_check_counters(ctx))) return rc;
    const size_t lds = row_words * 8;
    TLS_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(tlsdev::tls_remove_transits_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    TLS_HIP(ctx, hipMemcpyAsync(d_t, t, nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_cand, sorted.data(), m * sizeof(tlsdev::RemoveCandidate), hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_offset, offset.data(), (nc + 1) * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_profile, profile, table * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_sub, sub, (size_t)n_sub * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    for (size_t c0 = 0; c0 < nc; c0 += slab) {
        const size_t curves = std::min(slab, nc - c0);
        tlsdev::RemoveArgs a;
        a.t = d_t; a.cand = d_cand; a.offset = d_offset + c0;
        a.profile = d_profile; a.sub = d_sub; a.rows = d_rows; a.model = out_model ? d_model : nullptr; a.check = ctx->d_check.ptr;
        a.n = (long long)n; a.tiles_per_curve = (long long)((nn + tlsdev::kRemoveThreads - 1) / tlsdev::kRemoveThreads);
        a.tiles = (long long)curves * a.tiles_per_curve; a.nK = (int)n_k; a.M = (int)M; a.S = (int)n_sub;
        TLS_HIP(ctx, hipMemcpyAsync(d_rows, y + c0 * nn, curves * nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
        const unsigned blocks = (unsigned)std::min<long long>(a.tiles, 65536);
        hipLaunchKernelGGL(tlsdev::tls_remove_transits_kernel, dim3(blocks), dim3(tlsdev::kRemoveThreads), lds, main_stream(ctx), a);
        TLS_HIP(ctx, hipGetLastError());
        ctx->last_kernel = "tls_remove_transits";
        TLS_HIP(ctx, hipMemcpyAsync(out_rows + c0 * nn, d_rows, curves * nn * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        if (out_model) TLS_HIP(ctx, hipMemcpyAsync(out_model + c0 * nn, d_model, curves * nn * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        // (the next slab overwrites the device rows, and the grouped candidates live on this stack)
        TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));
    }
    return TLS_OK;
}

int tls_sysrem(tls_ctx* ctx, const double* y, const double* dy, int64_t n, int64_t n_rows, int64_t n_components,
               int64_t max_iter, double tol, double* out_flat, double* out_trend, double* out_c, double* out_a,
               int64_t* out_iters) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (n < 1 || n > 100000000) return fail(ctx, TLS_E_ARG, "sysrem: n out of range [1, 1e8]");
    if (n_rows < 2) return fail(ctx, TLS_E_ARG, "sysrem: n_rows < 2 (the fit runs across the rows)");
    if (n_components < 1 || n_components > std::min<int64_t>(TLS_SYSREM_MAX_COMPONENTS, n_rows - 1))
        return fail(ctx, TLS_E_ARG, "sysrem: n_components out of range [1, min(" + std::to_string(TLS_SYSREM_MAX_COMPONENTS) +
                                        ", n_rows - 1)]");
    if (max_iter < 1 || max_iter > TLS_SYSREM_MAX_ITER)
        return fail(ctx, TLS_E_ARG, "sysrem: max_iter out of range [1, " + std::to_string(TLS_SYSREM_MAX_ITER) + "]");
    if (!(std::isfinite(tol) && tol >= 0.0)) return fail(ctx, TLS_E_ARG, "sysrem: tol must be finite and >= 0");
    if (!y || !out_flat) return fail(ctx, TLS_E_ARG, "null argument");
    if ((uint64_t)n_rows > (uint64_t)(SIZE_MAX / 64) / (uint64_t)n) return fail(ctx, TLS_E_ARG, "sysrem: rows too large");
    const size_t nn = (size_t)n, R = (size_t)n_rows, K = (size_t)n_components, cells = R * nn;
    for (size_t q = 0; q < cells; ++q)
        if (!(std::isfinite(y[q]) && y[q] > 0.0))
            return fail(ctx, TLS_E_ARG, "sysrem: row " + std::to_string(q / nn) + " has a non-finite or non-positive value");
    if (dy)
        for (size_t q = 0; q < cells; ++q)
            if (!(std::isfinite(dy[q]) && dy[q] > 0.0))
                return fail(ctx, TLS_E_ARG, "sysrem: dy of row " + std::to_string(q / nn) + " has a non-finite or non-positive value");
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t chunks = (R + TLS_SYSREM_ROW_CHUNK - 1) / TLS_SYSREM_ROW_CHUNK;
    TLS_HIP(ctx, ctx->d_sysrem_state.reserve(tlsdev::kSysremState));
    double *d_y, *d_dy;
    tlsdev::SysremArgs a;
    Arena L;
    L.add(d_y, cells);  L.add(a.x, cells);  L.add(a.flat, cells);  L.add(d_dy, dy ? cells : 0);
    L.add(a.w, dy ? cells : R);   // (without dy: one weight a row)
    L.add(a.trend, out_trend ? cells : 0);  L.add(a.m, R);  L.add(a.c, K * R);  L.add(a.a, K * nn);
    L.add(a.pnum, chunks * nn);   // chunk partials
    L.add(a.pden, chunks * nn);
    TLS_HIP(ctx, L.bind(ctx->d_sysrem));
    a.y = d_y; a.dy = d_dy;
    a.state = ctx->d_sysrem_state.ptr; a.check = nullptr;
    a.n = (long long)n; a.rows = (long long)n_rows; a.chunks = (long long)chunks;
    a.tol = tol; a.n_components = (int)n_components; a.k = 0; a.iter = 0;
#ifdef TLS_DEBUG_CHECKS
    if (int rc = ensure_check_counters(ctx)) return rc;
    a.check = ctx->d_check.ptr;
#endif
    // one submission: the uploads, every launch of every component and the downloads, then one wait
    TLS_HIP(ctx, hipMemsetAsync(a.state, 0, tlsdev::kSysremState * sizeof(unsigned long long), main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_y, y, cells * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    if (dy) TLS_HIP(ctx, hipMemcpyAsync(d_dy, dy, cells * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    const dim3 block(tlsdev::kSysremLanes);
    const unsigned tiles = (unsigned)((nn + tlsdev::kSysremLanes - 1) / tlsdev::kSysremLanes);
    const dim3 by_row((unsigned)R), by_column(tiles);
    const dim3 by_chunk(tiles, (unsigned)std::min<size_t>(chunks, 65535)), by_cell(tiles, (unsigned)std::min<size_t>(R, 65535));
    hipLaunchKernelGGL(tlsdev::tls_sysrem_prepare, by_row, block, 0, main_stream(ctx), a);
    for (int k = 0; k < (int)n_components; ++k) {
        a.k = k;
        for (int it = 1; it <= (int)max_iter; ++it) {
            a.iter = it;
            hipLaunchKernelGGL(tlsdev::tls_sysrem_columns, by_chunk, block, 0, main_stream(ctx), a);
            hipLaunchKernelGGL(tlsdev::tls_sysrem_epochs, by_column, block, 0, main_stream(ctx), a);
            hipLaunchKernelGGL(tlsdev::tls_sysrem_rows, by_row, block, 0, main_stream(ctx), a);
        }
        TLS_HIP(ctx, hipGetLastError());
        if (k + 1 < (int)n_components) hipLaunchKernelGGL(tlsdev::tls_sysrem_subtract, by_cell, block, 0, main_stream(ctx), a);
    }
    hipLaunchKernelGGL(tlsdev::tls_sysrem_apply, by_cell, block, 0, main_stream(ctx), a);
    TLS_HIP(ctx, hipGetLastError());
    ctx->last_kernel = "tls_sysrem_apply";
    unsigned long long state[tlsdev::kSysremState];
    std::vector<double> c_rows(out_c ? K * R : 0);
    TLS_HIP(ctx, hipMemcpyAsync(out_flat, a.flat, cells * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
    if (out_trend) TLS_HIP(ctx, hipMemcpyAsync(out_trend, a.trend, cells * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
    if (out_c) TLS_HIP(ctx, hipMemcpyAsync(c_rows.data(), a.c, K * R * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
    if (out_a) TLS_HIP(ctx, hipMemcpyAsync(out_a, a.a, K * nn * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(state, a.state, sizeof state, hipMemcpyDeviceToHost, main_stream(ctx)));
    TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));
    if (state[tlsdev::kSysremBad]) {
        const unsigned long long first = ~state[tlsdev::kSysremBad];
        return fail(ctx, TLS_E_ARG, "sysrem: the trend of row " + std::to_string(first / nn) + ", point " +
                                        std::to_string(first % nn) + " is not finite and > 0 (the fit overshoots: check dy)");
    }
    if (out_c)   // (the device keeps one row per component)
        for (size_t i = 0; i < R; ++i)
            for (size_t k = 0; k < K; ++k) out_c[i * K + k] = c_rows[k * R + i];
    if (out_iters)
        for (size_t k = 0; k < K; ++k) out_iters[k] = (int64_t)state[tlsdev::kSysremIters + k];
    return TLS_OK;
}

int tls_spectra(tls_ctx* ctx, const double* chi2, int64_t n, int64_t kernel, double* out_SR, double* out_power_raw,
                double* out_power, double* out_sde) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (!out_SR || !out_power_raw || !out_power || !out_sde) return fail(ctx, TLS_E_ARG, "null output");
    // ((32 + kernel) doubles of dynamic LDS per median workgroup must stay within the 64 KB a launch gets without asking)
    if (kernel < 1 || kernel > 8000) return fail(ctx, TLS_E_ARG, "median kernel out of range [1, 8000]");
    if (!chi2 && !(ctx->executed && ctx->plan.n_periods > 0)) return fail(ctx, TLS_E_STATE, "tls_spectra without chi2 needs a finished search");
    if (chi2 && (n < 1 || n > 100000000)) return fail(ctx, TLS_E_ARG, "n out of range");
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    if (!chi2) n = ctx->plan.n_periods;
    if (kernel % 2 == 0) kernel += 1;                                   // stats.py:115-117
    const size_t nn = (size_t)n;
    tlsdev::SpectraArgs a;
    double* d_copy;   // the caller's chi2
    Arena L;
    L.add(a.SR, nn);  L.add(a.power_raw, nn);  L.add(a.power, nn);  L.add(a.sde, 2);  L.add(d_copy, nn);
    TLS_HIP(ctx, L.bind(ctx->d_spec));
    if (chi2) TLS_HIP(ctx, hipMemcpyAsync(d_copy, chi2, nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    a.chi2 = chi2 ? d_copy : ctx->d_chi2.ptr;
    a.n = (int)n; a.kernel = (int)kernel; a.detrend = n > 2 * kernel ? 1 : 0;
    a.chi2_stride = 0; a.out_stride = 0; a.sde_stride = 0;
    hipLaunchKernelGGL(tlsdev::tls_spectra_head, dim3(1), dim3(1024), 0, main_stream(ctx), a);
    if (a.detrend) {
        const int n_med = (int)(n - kernel + 1), threads = 256, per = tlsdev::kMedianWindows;
        const size_t lds = (size_t)(2 * per + kernel) * 8;
        hipLaunchKernelGGL(tlsdev::tls_spectra_median, dim3((unsigned)((n_med + per - 1) / per)), dim3(threads), lds,
                           main_stream(ctx), a);
        hipLaunchKernelGGL(tlsdev::tls_spectra_tail, dim3(1), dim3(1024), 0, main_stream(ctx), a);
    }
    TLS_HIP(ctx, hipGetLastError());
    if (out_power_raw == out_SR + nn && out_power == out_power_raw + nn && out_sde == out_power + nn) {
        // the caller's four outputs are one block, like the device's: one copy instead of four
        TLS_HIP(ctx, hipMemcpyAsync(out_SR, a.SR, (3 * nn + 2) * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
    } else {
        TLS_HIP(ctx, hipMemcpyAsync(out_SR, a.SR, nn * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        TLS_HIP(ctx, hipMemcpyAsync(out_power_raw, a.power_raw, nn * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        TLS_HIP(ctx, hipMemcpyAsync(out_power, a.power, nn * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        TLS_HIP(ctx, hipMemcpyAsync(out_sde, a.sde, 16, hipMemcpyDeviceToHost, main_stream(ctx)));
    }
    TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));
    return TLS_OK;
}

int tls_debug_folded(tls_ctx* ctx, double* out, int64_t capacity) {
    if (!ctx || !out) return fail(ctx, TLS_E_ARG, "bad argument");
    if (!ctx->prepared) return fail(ctx, TLS_E_STATE, "tls_debug_folded before tls_prepare");
    const int64_t need = ctx->plan.n_periods * ctx->plan.n;
    if (capacity < need) return fail(ctx, TLS_E_ARG, "tls_debug_folded: out holds fewer than n_periods * n doubles");
    if (need == 0) return TLS_OK;
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    BufPool local;   // (freed at scope exit, on every path)
    DevBuf<double> d_out(local, "d_out", kScratch);
    TLS_HIP(ctx, d_out.reserve((size_t)need));
    int rc = enqueue(ctx, false, false, d_out.ptr);
    if (rc == TLS_OK) {
        ctx->executed = true;
        hipError_t e = hipMemcpyAsync(out, d_out.ptr, (size_t)need * 8, hipMemcpyDeviceToHost, main_stream(ctx));
        if (e == hipSuccess) e = hipStreamSynchronize(main_stream(ctx));
        if (e != hipSuccess) rc = fail(ctx, TLS_E_HIP, hipGetErrorString(e));
    }
    if (rc != TLS_OK) (void)hipStreamSynchronize(main_stream(ctx));
    return rc;
}

int tls_debug_prefix(tls_ctx* ctx, double* out, int64_t capacity, int64_t* row_length) {
    if (!ctx || !row_length) return fail(ctx, TLS_E_ARG, "bad argument");
    if (!ctx->prepared) return fail(ctx, TLS_E_STATE, "tls_debug_prefix before tls_prepare");
    *row_length = ctx->plan.M + 1;
    if (!out) return TLS_OK;   // size query
    const int64_t need = ctx->plan.n_periods * (ctx->plan.M + 1);
    if (capacity < need) return fail(ctx, TLS_E_ARG, "tls_debug_prefix: out holds fewer than n_periods * row_length doubles");
    if (need == 0) return TLS_OK;
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    BufPool local;   // (freed at scope exit, on every path)
    DevBuf<double> d_out(local, "d_out", kScratch);
    TLS_HIP(ctx, d_out.reserve((size_t)need));
    int rc = enqueue(ctx, false, false, nullptr, d_out.ptr);
    if (rc == TLS_OK) {
        ctx->executed = true;
        hipError_t e = hipMemcpyAsync(out, d_out.ptr, (size_t)need * 8, hipMemcpyDeviceToHost, main_stream(ctx));
        if (e == hipSuccess) e = hipStreamSynchronize(main_stream(ctx));
        if (e != hipSuccess) rc = fail(ctx, TLS_E_HIP, hipGetErrorString(e));
    }
    if (rc != TLS_OK) (void)hipStreamSynchronize(main_stream(ctx));
    return rc;
}

int tls_debug_period_cycles(tls_ctx* ctx, uint64_t* cycles, int64_t capacity) {
    if (!ctx || !cycles) return fail(ctx, TLS_E_ARG, "bad argument");
    if (!ctx->prepared) return fail(ctx, TLS_E_STATE, "tls_debug_period_cycles before tls_prepare");
    if (capacity < ctx->plan.n_periods) return fail(ctx, TLS_E_ARG, "tls_debug_period_cycles: out holds fewer than n_periods entries");
    if (ctx->plan.n_periods == 0) return TLS_OK;
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    BufPool local;   // (freed at scope exit, on every path)
    DevBuf<unsigned long long> d_out(local, "d_out", kScratch);
    TLS_HIP(ctx, d_out.reserve((size_t)ctx->plan.n_periods));
    hipError_t e = hipMemsetAsync(d_out.ptr, 0, (size_t)ctx->plan.n_periods * 8, main_stream(ctx));
    int rc = e == hipSuccess ? enqueue(ctx, false, false, nullptr, nullptr, d_out.ptr) : fail(ctx, TLS_E_HIP, hipGetErrorString(e));
    if (rc == TLS_OK) {
        e = hipMemcpyAsync(cycles, d_out.ptr, (size_t)ctx->plan.n_periods * 8, hipMemcpyDeviceToHost, main_stream(ctx));
        if (e == hipSuccess) e = hipStreamSynchronize(main_stream(ctx));
        if (e != hipSuccess) rc = fail(ctx, TLS_E_HIP, hipGetErrorString(e));
    } else {
        (void)hipStreamSynchronize(main_stream(ctx));
    }
    return rc;
}

int tls_debug_cumsum(tls_ctx* ctx, const double* f, int64_t count, double* out, int threads) {
    if (!ctx || !f || !out || count < 0 || count > 100000000) return fail(ctx, TLS_E_ARG, "bad argument");
    if (threads < 64 || threads > 1024 || threads % 64) return fail(ctx, TLS_E_ARG, "threads must be a multiple of 64 in [64, 1024]");
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    BufPool local;   // (freed at scope exit, on every path)
    DevBuf<double> d_f(local, "d_f", kScratch), d_out(local, "d_out", kScratch);
    TLS_HIP(ctx, d_f.reserve((size_t)count));
    TLS_HIP(ctx, d_out.reserve((size_t)count + 1));
    if (count) TLS_HIP(ctx, hipMemcpyAsync(d_f.ptr, f, (size_t)count * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    const int variant = 0;   // (1: the first version of the routine, kept in the kernel for A/B builds)
    // block / fallback counts of this call land in the phase-clock buffer (tls_debug_phase_cycles slots 10, 11)
    TLS_HIP(ctx, ctx->d_phase.reserve(tlsdev::kPhases));
    TLS_HIP(ctx, hipMemsetAsync(ctx->d_phase.ptr, 0, tlsdev::kPhases * sizeof(unsigned long long), main_stream(ctx)));
    { const unsigned long long big = ~0ull; TLS_HIP(ctx, hipMemcpyAsync(ctx->d_phase.ptr + 22, &big, 8, hipMemcpyHostToDevice, main_stream(ctx))); TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx))); }
    hipLaunchKernelGGL(tlsdev::tls_cumsum_kernel, dim3(1), dim3((unsigned)threads), 0, main_stream(ctx), d_f.ptr, d_out.ptr, (int)count, variant, ctx->d_phase.ptr);
    TLS_HIP(ctx, hipGetLastError());
    TLS_HIP(ctx, hipMemcpyAsync(out, d_out.ptr, ((size_t)count + 1) * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
    TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));
    return TLS_OK;
}

int tls_debug_phase_cycles(tls_ctx* ctx, uint64_t* cycles, int n) {
    if (!ctx || !cycles || n < 1) return fail(ctx, TLS_E_ARG, "bad argument");
    if (!ctx->d_phase.ptr) return fail(ctx, TLS_E_STATE, "no execute with the phase clock (count_work & 2)");
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));
    unsigned long long host[tlsdev::kPhases];
    TLS_HIP(ctx, hipMemcpy(host, ctx->d_phase.ptr, sizeof host, hipMemcpyDeviceToHost));
    for (int i = 0; i < n && i < tlsdev::kPhases; ++i) cycles[i] = host[i];
    return TLS_OK;
}

namespace {
// test entry: every byte of every CU's LDS set to a pattern (one workgroup with all 160 KB per CU, a few rounds of them)
__global__ void __launch_bounds__(1024) tls_poison_lds_kernel(unsigned int word, unsigned int* sink) {
    extern __shared__ unsigned int lds_words[];
    const unsigned int total = 160u * 1024u / 4u;
    for (unsigned int k = threadIdx.x; k < total; k += blockDim.x) lds_words[k] = word;
    tlsdev::wg_sync();
    if (lds_words[(threadIdx.x * 97u) % total] != word && sink) sink[0] = 1u;   // (keeps the stores alive)
}
}  // namespace

int tls_debug_poison_lds(tls_ctx* ctx, uint32_t word) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    TLS_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(tls_poison_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipLaunchKernelGGL(tls_poison_lds_kernel, dim3((unsigned)(4 * ctx->n_cu)), dim3(1024), 160 * 1024, main_stream(ctx), (unsigned int)word,
                       static_cast<unsigned int*>(nullptr));
    TLS_HIP(ctx, hipGetLastError());
    // ... and every scratch buffer of the context (the per-workgroup scratch in HBM, the T0 fit's slabs, the post-search
    // chain's arrays, every survey stage's buffer): all ones -- NaNs as doubles -- as fresh device memory may be.  What a
    // state buffer holds between calls is state by design; the reason stands beside each in tls_ctx.
    for (const tlsmem::PoolBuf* b = ctx->pool.first; b; b = b->next)
        if (b->kind == kScratch && b->base() && b->cap) TLS_HIP(ctx, hipMemsetAsync(b->base(), 0xFF, b->bytes(), main_stream(ctx)));
    return TLS_OK;
}

int tls_debug_batch_group_ms(const tls_ctx* ctx, double* out, int64_t capacity) {
    if (!ctx) return TLS_E_ARG;
    const int64_t n = (int64_t)ctx->batch_group_ms.size();
    if (out) {
        for (int64_t i = 0; i < std::min(n, capacity); ++i) out[i] = ctx->batch_group_ms[(size_t)i];
        // (capacity for twice the groups: the second half is the part of each group's time spent in its wait for the device)
        const int64_t nw = (int64_t)ctx->batch_group_wait_ms.size();
        for (int64_t i = 0; i < nw && n + i < capacity; ++i) out[n + i] = ctx->batch_group_wait_ms[(size_t)i];
    }
    return (int)std::min<int64_t>(n, 0x7fffffff);
}

int tls_debug_post_search(tls_ctx* ctx, const double* y, int64_t n_curves, const double* chi2, const int64_t* row,
                          const double* depth, int64_t median_kernel, tls_power_summary* out_summary, double* out_epochs,
                          double* out_residuals, int64_t* out_n_epochs, int64_t* out_handed_back) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (!ctx->prepared || !ctx->key.valid) return fail(ctx, TLS_E_STATE, "tls_debug_post_search before tls_prepare");
    if (!y || !chi2 || !row || !depth || !out_summary) return fail(ctx, TLS_E_ARG, "null argument");
    if (n_curves < 1 || n_curves > 1024) return fail(ctx, TLS_E_ARG, "n_curves out of range [1, 1024]");
    if (median_kernel < 1 || median_kernel > 8000) return fail(ctx, TLS_E_ARG, "median kernel out of range [1, 8000]");
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    const PlanKey& k = ctx->key;
    const int64_t n = k.n, n_periods = k.n_periods;
    if (n_periods < 1) return fail(ctx, TLS_E_ARG, "tls_debug_post_search needs at least one period");
    const double t_min = *std::min_element(k.t.begin(), k.t.end()), t_max = *std::max_element(k.t.begin(), k.t.end());
    const int64_t max_len = *std::max_element(k.length.begin(), k.length.end());
    const size_t np = (size_t)n_periods, nn = (size_t)n, gc = (size_t)n_curves;
    auto& sl = ctx->slot[0];
    TLS_HIP(ctx, sl.d_y.reserve(gc * nn));
    TLS_HIP(ctx, sl.d_chi2.reserve(gc * np));
    TLS_HIP(ctx, sl.d_row.reserve(gc * np));
    TLS_HIP(ctx, sl.d_depth.reserve(gc * np));
    PostSearchBufs pb;
    int rc = reserve_post_search(ctx, n_curves, n_periods, n, max_len, pb);
    if (rc) return rc;
    TLS_HIP(ctx, hipMemcpyAsync(sl.d_y.ptr, y, gc * nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(sl.d_chi2.ptr, chi2, gc * np * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(sl.d_row.ptr, row, gc * np * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(sl.d_depth.ptr, depth, gc * np * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    if ((rc = enqueue_post_search(ctx, pb, n_curves, sl.d_chi2.ptr, sl.d_row.ptr, sl.d_depth.ptr, sl.d_y.ptr, n, n_periods,
                                  median_kernel, t_min, t_max, k.params.T0_fit_margin))) {
        (void)hipStreamSynchronize(main_stream(ctx));
        return rc;
    }
    std::vector<double> h(11 * gc);
    TLS_HIP(ctx, hipMemcpyAsync(h.data(), pb.sde, 11 * gc * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
    std::vector<int> nep(gc);
    TLS_HIP(ctx, hipMemcpyAsync(nep.data(), pb.n_epochs, gc * sizeof(int), hipMemcpyDeviceToHost, main_stream(ctx)));
    if (out_epochs) TLS_HIP(ctx, hipMemcpyAsync(out_epochs, ctx->d_fep.ptr, gc * nn * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
    if (out_residuals) TLS_HIP(ctx, hipMemcpyAsync(out_residuals, ctx->d_fres.ptr, gc * nn * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
    // (the rotation path's flag of every fit: state[1] behind the base order's three arrays, launch_t0_fit's layout)
    const bool rotation = ctx->opt.t0_rot != 0 && n >= tlsdev::kT0RotMinPoints;
    std::vector<double> flag(gc, -1.0);
    if (out_handed_back && rotation)
        TLS_HIP(ctx, hipMemcpy2DAsync(flag.data(), 8, ctx->d_frot.ptr + 3 * nn + 1, (3 * nn + 4) * 8, 8, gc, hipMemcpyDeviceToHost, main_stream(ctx)));
    TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));
    for (size_t c = 0; c < gc; ++c) {
        if (out_n_epochs) out_n_epochs[c] = nep[c];
        // (a fit with no trial epoch never ran: its slot of the rotation path holds nothing of it)
        if (out_handed_back) out_handed_back[c] = !rotation ? -1 : nep[c] < 1 ? 0 : flag[c] != 0.0 ? 1 : 0;
    }
    ctx->executed = false;   // (the batch slot's buffers were written: as after tls_power_batch)
    for (int64_t c = 0; c < n_curves; ++c)
        if ((rc = read_summary(ctx, h.data(), n_curves, c, c, out_summary[c]))) return rc;
    return TLS_OK;
}

// tls_debug_transit_stats, and with `mr` tls_debug_transit_models: the statistics stage (then the models) on injected picks
static int debug_transit_impl(tls_ctx* ctx, const double* y, int64_t n_curves, const double* period, const double* T0,
                              const int64_t* best_row, const double* depth, const int64_t* no_fit, const int64_t* index_power,
                              const double* power, const double* row_duration, int64_t n_rows, double fill_factor,
                              const double* root, const double* root_count, int64_t n_root, int64_t max_epochs,
                              tls_transit_stats* out_stats,
                              double* out_per_transit, int64_t* out_n_epochs, const ModelsRequest* mr) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (!ctx->prepared || !ctx->key.valid) return fail(ctx, TLS_E_STATE, "tls_debug_transit_stats before tls_prepare");
    if (!y || !period || !T0 || !best_row || !depth || !no_fit || !index_power || !power) return fail(ctx, TLS_E_ARG, "null argument");
    if (n_curves < 1 || n_curves > 1024) return fail(ctx, TLS_E_ARG, "n_curves out of range [1, 1024]");
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    const PlanKey& k = ctx->key;
    const int64_t n = k.n, n_periods = k.n_periods;
    if (n_periods < 1) return fail(ctx, TLS_E_ARG, "tls_debug_transit_stats needs at least one period");
    const StatsRequest sr = stats_request(row_duration, n_rows, fill_factor, root, root_count, n_root, max_epochs, out_stats,
                                          out_per_transit,
                                          out_n_epochs);
    int rc = check_stats_request(ctx, sr, k.t.data(), n, k.n_rows);
    if (rc || (mr && (rc = check_models_request(ctx, *mr, n)))) return rc;
    const size_t np = (size_t)n_periods, nn = (size_t)n, gc = (size_t)n_curves;
    for (size_t c = 0; c < gc; ++c) {
        if (index_power[c] < 0 || index_power[c] >= n_periods) return fail(ctx, TLS_E_ARG, "index_power out of range");
        if (!no_fit[c] && (best_row[c] < 0 || best_row[c] >= n_rows)) return fail(ctx, TLS_E_ARG, "best_row out of range");
    }
    const double t_min = *std::min_element(k.t.begin(), k.t.end()), t_max = *std::max_element(k.t.begin(), k.t.end());
    auto& sl = ctx->slot[0];
    TLS_HIP(ctx, sl.d_y.reserve(gc * nn));
    PostSearchBufs pb;
    if ((rc = reserve_post_search(ctx, n_curves, n_periods, n, 1, pb, sr.words()))) return rc;
    StatsBufs sb;
    if ((rc = reserve_transit_stats(ctx, sr, n_curves, n, sb))) return rc;
    ModelsBufs mb;
    if (mr && (rc = reserve_transit_models(ctx, *mr, n_curves, n, mb))) return rc;
    // the pick record of tls_power_pick ([2] index_power, [3] period, [4] depth, [5] best_row, [6] no_fit) and T0
    std::vector<double> pick(8 * gc + gc, 0.0);
    for (size_t c = 0; c < gc; ++c) {
        double* pk = pick.data() + 8 * c;
        pk[2] = (double)index_power[c]; pk[3] = period[c]; pk[4] = depth[c]; pk[5] = (double)(no_fit[c] ? 0 : best_row[c]);
        pk[6] = no_fit[c] ? 1.0 : 0.0;
        pick[8 * gc + c] = T0[c];
    }
    TLS_HIP(ctx, hipMemcpyAsync(sl.d_y.ptr, y, gc * nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpy2DAsync(ctx->d_spec.ptr + 2 * np, pb.spec_stride * 8, power, np * 8, np * 8, gc, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(pb.pick, pick.data(), pick.size() * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    if ((rc = enqueue_transit_stats(ctx, pb, sb, sr, n_curves, sl.d_y.ptr, n, n_periods, t_min, t_max))) {
        (void)hipStreamSynchronize(main_stream(ctx));
        return rc;
    }
    if (mr && (rc = enqueue_transit_models(ctx, pb, sb, sr, *mr, mb, n_curves, sl.d_y.ptr, n, t_min, t_max))) {
        (void)hipStreamSynchronize(main_stream(ctx));
        return rc;
    }
    std::vector<double> h(gc * sr.words()), hm(mr ? gc * mb.out_stride : 0);
    TLS_HIP(ctx, hipMemcpyAsync(h.data(), pb.stats, h.size() * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
    if (mr) TLS_HIP(ctx, hipMemcpyAsync(hm.data(), mb.out, hm.size() * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
    TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));
    ctx->executed = false;   // (the batch slot's buffers were written: as after tls_power_batch)
    for (int64_t c = 0; c < n_curves; ++c)
        if ((rc = read_transit_stats(ctx, sr, h.data(), n_curves, c, c, true))) return rc;
    if (mr)
        for (int64_t c = 0; c < n_curves; ++c)
            if ((rc = read_transit_models(ctx, *mr, hm.data(), mb.out_stride, c, c, n))) return rc;
    return TLS_OK;
}

int tls_debug_transit_stats(tls_ctx* ctx, const double* y, int64_t n_curves, const double* period, const double* T0,
                            const int64_t* best_row, const double* depth, const int64_t* no_fit, const int64_t* index_power,
                            const double* power, const double* row_duration, int64_t n_rows, double fill_factor,
                            const double* root, const double* root_count, int64_t n_root, int64_t max_epochs,
                            tls_transit_stats* out_stats,
                            double* out_per_transit, int64_t* out_n_epochs) {
    return debug_transit_impl(ctx, y, n_curves, period, T0, best_row, depth, no_fit, index_power, power, row_duration, n_rows,
                              fill_factor, root, root_count, n_root, max_epochs, out_stats, out_per_transit, out_n_epochs, nullptr);
}

int tls_debug_transit_models(tls_ctx* ctx, const double* y, int64_t n_curves, const double* period, const double* T0,
                             const int64_t* best_row, const double* depth, const int64_t* no_fit, const int64_t* index_power,
                             const double* power, const double* row_duration, int64_t n_rows, double fill_factor,
                             const double* root, const double* root_count, int64_t n_root, int64_t max_epochs,
                             tls_transit_stats* out_stats,
                             double* out_per_transit, int64_t* out_n_epochs, const double* curve_t, const double* curve_f,
                             int64_t curve_n, double curve_lo, double curve_hi, double maxw, int64_t lc_cap,
                             double* out_folded, double* out_model_folded, double* out_lc, int64_t* out_lc_len) {
    const ModelsRequest mr = models_request(curve_t, curve_f, curve_n, curve_lo, curve_hi, maxw, lc_cap, out_folded,
                                            out_model_folded, out_lc, out_lc_len);
    return debug_transit_impl(ctx, y, n_curves, period, T0, best_row, depth, no_fit, index_power, power, row_duration, n_rows,
                              fill_factor, root, root_count, n_root, max_epochs, out_stats, out_per_transit, out_n_epochs, &mr);
}

// tls_debug_peak_fits; ps: tls_debug_peak_phase_scans, the fits' phase scans as well
static int debug_peak_fits_impl(tls_ctx* ctx, const double* y, int64_t n_curves, const tls_peak* peaks, const int64_t* n_peaks,
                                int64_t k, const double* power, const double* row_duration, int64_t n_rows, double fill_factor,
                                const double* root, const double* root_count, int64_t n_root, int64_t max_epochs,
                                tls_peak_fit* out_fits, double* out_epochs,
                                double* out_residuals, int64_t* out_n_epochs, const PhaseScanRequest* ps) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (!ctx->prepared || !ctx->key.valid) return fail(ctx, TLS_E_STATE, "tls_debug_peak_fits before tls_prepare");
    if (!y || !peaks || !n_peaks || !power || !out_fits) return fail(ctx, TLS_E_ARG, "null argument");
    if (n_curves < 1 || n_curves > 1024) return fail(ctx, TLS_E_ARG, "n_curves out of range [1, 1024]");
    if (k < 1 || k > TLS_PEAKS_MAX_K) return fail(ctx, TLS_E_ARG, "peaks: k out of range [1, 32]");
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    const PlanKey& key = ctx->key;
    const int64_t n = key.n, n_periods = key.n_periods;
    if (n_periods < 1) return fail(ctx, TLS_E_ARG, "tls_debug_peak_fits needs at least one period");
    const StatsRequest sr = stats_request(row_duration, n_rows, fill_factor, root, root_count, n_root, max_epochs, nullptr,
                                          nullptr, nullptr);
    int rc = check_stats_request(ctx, sr, key.t.data(), n, key.n_rows, false);
    if (rc) return rc;
    const size_t np = (size_t)n_periods, nn = (size_t)n, gc = (size_t)n_curves, kk = (size_t)k;
    PeaksRequest pk;
    pk.k = k;
    // the records as tls_find_peaks leaves them: n_peaks | k records of six words
    std::vector<unsigned long long> rec(gc * pk.words());
    for (size_t c = 0; c < gc; ++c) {
        if (n_peaks[c] < 0 || n_peaks[c] > k) return fail(ctx, TLS_E_ARG, "n_peaks out of range [0, k]");
        for (int64_t r = 0; r < n_peaks[c]; ++r) {
            const tls_peak& p = peaks[c * kk + (size_t)r];
            if (p.index < 0 || p.index >= n_periods) return fail(ctx, TLS_E_ARG, "peak index out of range");
            if (p.row < -1 || p.row >= n_rows) return fail(ctx, TLS_E_ARG, "peak row out of range");
        }
        rec[c * pk.words()] = (unsigned long long)n_peaks[c];
        std::memcpy(&rec[c * pk.words() + 1], peaks + c * kk, kk * sizeof(tls_peak));
    }
    const double t_min = *std::min_element(key.t.begin(), key.t.end()), t_max = *std::max_element(key.t.begin(), key.t.end());
    const int64_t max_len = *std::max_element(key.length.begin(), key.length.end());
    PeakFitsRequest pf;
    pf.k = k; pf.inputs = &sr; pf.out = out_fits;
    pf.out_epochs = out_epochs; pf.out_residuals = out_residuals; pf.out_n_epochs = out_n_epochs;
    auto& sl = ctx->slot[0];
    TLS_HIP(ctx, sl.d_y.reserve(gc * nn));
    PostSearchBufs pb;
    const size_t scans_out = ps ? (size_t)tlsdev::kPhaseWords * kk : 0;
    if ((rc = reserve_post_search(ctx, n_curves, n_periods, n, max_len, pb, 0, pk.words(), 0, pf.words(), scans_out))) return rc;
    StatsBufs sb;
    if ((rc = reserve_transit_stats(ctx, sr, 0, n, sb))) return rc;
    PeakFitBufs fb;
    if ((rc = reserve_peak_fits(ctx, n_curves * k, n, max_len, max_epochs, fb))) return rc;
    TLS_HIP(ctx, hipMemcpyAsync(sl.d_y.ptr, y, gc * nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpy2DAsync(ctx->d_spec.ptr + 2 * np, pb.spec_stride * 8, power, np * 8, np * 8, gc, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(pb.peaks, rec.data(), rec.size() * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    if ((rc = enqueue_peak_fits(ctx, fb, pf, sb, n_curves, n_curves, pb.peaks, pb.fits, sl.d_y.ptr, ctx->d_spec.ptr + 2 * np,
                                pb.spec_stride, n, n_periods, t_min, t_max, key.params.T0_fit_margin, 0, ps, pb.scans))) {
        (void)hipStreamSynchronize(main_stream(ctx));
        return rc;
    }
    // (fits and scans lie side by side; fit f = c k + r: the scans are already in the caller's order)
    std::vector<double> h(gc * (pf.words() + scans_out));
    TLS_HIP(ctx, hipMemcpyAsync(h.data(), pb.fits, h.size() * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
    TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));
    ctx->executed = false;   // (the batch slot's buffers were written: as after tls_power_batch)
    for (int64_t c = 0; c < n_curves; ++c)
        if ((rc = read_peak_fits(ctx, pf, h.data(), n_curves, c, c))) return rc;
    if (ps) std::memcpy(ps->out, h.data() + gc * pf.words(), gc * scans_out * 8);
    return TLS_OK;
}

int tls_debug_peak_fits(tls_ctx* ctx, const double* y, int64_t n_curves, const tls_peak* peaks, const int64_t* n_peaks,
                        int64_t k, const double* power, const double* row_duration, int64_t n_rows, double fill_factor,
                        const double* root, const double* root_count, int64_t n_root, int64_t max_epochs, tls_peak_fit* out_fits,
                        double* out_epochs,
                        double* out_residuals, int64_t* out_n_epochs) {
    return debug_peak_fits_impl(ctx, y, n_curves, peaks, n_peaks, k, power, row_duration, n_rows, fill_factor, root, root_count,
                                n_root,
                                max_epochs, out_fits, out_epochs, out_residuals, out_n_epochs, nullptr);
}

int tls_debug_peak_phase_scans(tls_ctx* ctx, const double* y, int64_t n_curves, const tls_peak* peaks, const int64_t* n_peaks,
                               int64_t k, const double* power, const double* row_duration, int64_t n_rows, double fill_factor,
                               const double* root, const double* root_count, int64_t n_root, int64_t max_epochs,
                               tls_peak_fit* out_fits,
                               int64_t max_bins, int64_t min_count, tls_phase_record* out_scans) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (!out_scans) return fail(ctx, TLS_E_ARG, "null argument");
    PhaseScanRequest ps;
    ps.max_bins = max_bins; ps.min_count = min_count; ps.out = out_scans;
    const int rc = check_phase_scan_request(ctx, ps);
    if (rc) return rc;
    return debug_peak_fits_impl(ctx, y, n_curves, peaks, n_peaks, k, power, row_duration, n_rows, fill_factor, root, root_count,
                                n_root,
                                max_epochs, out_fits, nullptr, nullptr, nullptr, &ps);
}

int tls_debug_device_bytes(const tls_ctx* ctx, int64_t* total, int64_t* t0_fit_scratch) {
    if (!ctx || !total || !t0_fit_scratch) return TLS_E_ARG;
    *total = (int64_t)ctx->pool.bytes();
    *t0_fit_scratch = (int64_t)(ctx->d_fscratch.cap * sizeof(double));
    return TLS_OK;
}

int tls_debug_lanes(const tls_ctx* ctx, int64_t* lane_a, int64_t* lane_b, int64_t* on) {
    if (!ctx || !lane_a || !lane_b) return TLS_E_ARG;
    *lane_a = ctx->lane_launches[0]; *lane_b = ctx->lane_launches[1];
    if (on) *on = ctx->lanes != 0 ? 1 : 0;
    return TLS_OK;
}

int tls_debug_perm_table(const tls_ctx* ctx, int64_t* bytes, int64_t* filled, int64_t* plan_reuses) {
    if (!ctx || !bytes || !filled) return TLS_E_ARG;
    if (plan_reuses) *plan_reuses = ctx->plan_reuses;
    *bytes = (int64_t)(ctx->perm_table_entries * sizeof(unsigned short));
    *filled = ctx->perm_table_entries && ctx->perm_filled ? 1 : 0;
    return TLS_OK;
}

int tls_debug_check_counts(tls_ctx* ctx, uint64_t* counts, int n) {
    if (!ctx || !counts || n < 1) return fail(ctx, TLS_E_ARG, "bad argument");
    for (int i = 0; i < n; ++i) counts[i] = 0;
#ifdef TLS_DEBUG_CHECKS
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));
    if (ctx->d_check.ptr) {
        unsigned long long host[tlsdev::kChecks];
        TLS_HIP(ctx, hipMemcpy(host, ctx->d_check.ptr, sizeof host, hipMemcpyDeviceToHost));
        for (int i = 0; i < n && i < tlsdev::kChecks; ++i) counts[i] = host[i];
    }
    return 1;   // a checked build
#else
    return TLS_OK;   // not a checked build: all zero
#endif
}

int tls_synchronize(tls_ctx* ctx) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->lane_b.stream) TLS_HIP(ctx, hipStreamSynchronize(ctx->lane_b.stream));   // (both lanes)
    TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));
    return TLS_OK;
}

int tls_execute_timed(tls_ctx* ctx, int reps, double* ms_per_execute) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (!ctx->prepared) return fail(ctx, TLS_E_STATE, "tls_execute_timed before tls_prepare");
    if (reps < 1 || !ms_per_execute) return fail(ctx, TLS_E_ARG, "reps must be >= 1");
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->plan.n_periods == 0) { *ms_per_execute = 0; return TLS_OK; }
    TLS_HIP(ctx, hipEventRecord(ctx->ev0, main_stream(ctx)));
    for (int r = 0; r < reps; ++r) {
        int rc = enqueue(ctx, false);
        if (rc) return rc;
    }
    TLS_HIP(ctx, hipEventRecord(ctx->ev1, main_stream(ctx)));
    TLS_HIP(ctx, hipEventSynchronize(ctx->ev1));
    float ms = 0;
    TLS_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    *ms_per_execute = (double)ms / reps;
    return TLS_OK;
}

int tls_fetch(tls_ctx* ctx, double* out_chi2, int64_t* out_row, double* out_depth, tls_counters* counters) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (!ctx->executed) return fail(ctx, TLS_E_STATE, "tls_fetch before tls_execute");
    if (!out_chi2 || !out_row || !out_depth) return fail(ctx, TLS_E_ARG, "null output");
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t np = (size_t)ctx->plan.n_periods;
    static_assert(sizeof(long long) == sizeof(int64_t), "int64 layout");
    unsigned long long dev_counts[3] = {0, 0, 0};
    if (np) {
        // [chi2 | row | depth | counters] leave the device as ONE copy into pinned memory
        const size_t words = 3 * np + 4;
        if (ctx->h_out_cap < words) {
            if (ctx->h_out) TLS_HIP(ctx, hipHostFree(ctx->h_out));
            ctx->h_out = nullptr; ctx->h_out_cap = 0;
            TLS_HIP(ctx, hipHostMalloc(reinterpret_cast<void**>(&ctx->h_out), (words + words / 4) * 8, hipHostMallocDefault));
            ctx->h_out_cap = words + words / 4;
        }
        TLS_HIP(ctx, hipMemcpyAsync(ctx->h_out, ctx->d_latest.ptr, words * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));
        std::memcpy(out_chi2, ctx->h_out, np * 8);
        std::memcpy(out_row, ctx->h_out + np, np * 8);
        std::memcpy(out_depth, ctx->h_out + 2 * np, np * 8);
        std::memcpy(dev_counts, ctx->h_out + 3 * np, sizeof dev_counts);
    } else {
        TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));
    }
    if (counters) {
        *counters = ctx->plan_counters;
        counters->evaluated_cells = ctx->counted ? (int64_t)dev_counts[0] : -1;
        counters->inner_steps = ctx->counted ? (int64_t)dev_counts[1] : -1;
        counters->issued_fma = ctx->counted ? (int64_t)dev_counts[2] : -1;
    }
    return TLS_OK;
}

namespace {
// what every launch in the event ring is charged, in ring order (both lanes waited for)
int launch_terms(tls_ctx* ctx, std::vector<double>& terms) {
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->lane_b.stream) TLS_HIP(ctx, hipStreamSynchronize(ctx->lane_b.stream));   // (both lanes)
    TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));
    const size_t n_timed = std::min(ctx->ev_used, ctx->ev_pool.size());
    terms.assign(n_timed, 0.0);
    // An overlapped launch's own pair starts when its marker runs -- up to a whole launch before its workgroups find room on
    // the device.  It is charged the shorter of its own pair and (end of the launch before it -> its own end), so that the sum
    // over a run of overlapped launches is the time the run took and the mean stays a per-search figure.
    const size_t oldest = ctx->ev_used > kEventRing ? ctx->ev_used % kEventRing : 0;   // (its predecessor's slot holds a newer launch)
    for (size_t i = 0; i < n_timed; ++i) {
        float ms = 0;
        TLS_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev_pool[i].first, ctx->ev_pool[i].second));
        if (ctx->ev_overlapped[i] && i != oldest) {
            float since_prev = 0;
            // (a launch that ended before its predecessor did keeps its own pair)
            if (hipEventElapsedTime(&since_prev, ctx->ev_pool[(i + kEventRing - 1) % kEventRing].second, ctx->ev_pool[i].second) != hipSuccess) {
                (void)hipGetLastError();
                since_prev = 0;
            }
            if (since_prev > 0 && since_prev < ms) ms = since_prev;
        }
        terms[i] = ms;
    }
    return TLS_OK;
}
}  // namespace

int tls_kernel_timing(tls_ctx* ctx, int reset, double* total_ms, int64_t* launches) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    std::vector<double> terms;
    if (int rc = launch_terms(ctx, terms)) return rc;
    double sum = 0;
    for (double ms : terms) sum += ms;
    if (total_ms) *total_ms = sum;
    if (launches) *launches = (int64_t)terms.size();
    if (reset) ctx->ev_used = 0;
    return TLS_OK;
}

int tls_debug_launch_ms(tls_ctx* ctx, double* out, int64_t capacity) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    std::vector<double> terms;
    if (int rc = launch_terms(ctx, terms)) return rc;
    if (out) for (size_t i = 0; i < terms.size() && (int64_t)i < capacity; ++i) out[i] = terms[i];
    return (int)terms.size();
}

const char* tls_last_kernel(const tls_ctx* ctx) { return ctx ? ctx->last_kernel : ""; }

int tls_plan_info(const tls_ctx* ctx, tls_counters* counters, int64_t* lds_bytes, int64_t* n_blocks, int64_t* resident) {
    if (!ctx || !ctx->prepared) return TLS_E_STATE;
    if (counters) { *counters = ctx->plan_counters; counters->evaluated_cells = -1; counters->inner_steps = -1; counters->issued_fma = -1; }
    // (the launch shape of the kernel a plain search of this plan takes)
    const bool slim = is_slim(pick_kernel(ctx->plan, ctx->flux));
    if (lds_bytes) *lds_bytes = (int64_t)(slim ? ctx->plan.slim_lds : ctx->plan.lds_bytes);
    if (n_blocks) *n_blocks = slim ? ctx->plan.slim_blocks : ctx->plan.blocks;
    if (resident) *resident = ctx->plan.resident ? 1 : 0;
    return TLS_OK;
}

int tls_search(tls_ctx* ctx, const double* t, const double* y, const double* dy, int64_t n, const double* periods,
               int64_t n_periods, const tls_template* tmpl, const tls_params* params, double* out_chi2,
               int64_t* out_row, double* out_depth, tls_counters* counters) {
    int rc = tls_prepare(ctx, t, y, dy, n, periods, n_periods, tmpl, params);
    if (rc) return rc;
    if ((rc = tls_execute(ctx, counters != nullptr))) return rc;
    return tls_fetch(ctx, out_chi2, out_row, out_depth, counters);
}

// the groups of tls_search_batch, pipelined over two slots of device and pinned host buffers: while group g is searched,
// group g+1 is formed on the host (weights, S0) and uploaded on a second stream, and the results of group g-1 travel back
// and are copied into the caller's arrays
static int search_batch_impl(tls_ctx* ctx, const double* y, const double* dy, int64_t n, int64_t n_curves, int64_t n_periods,
                             double* out_chi2, int64_t* out_row, double* out_depth) {
    const int64_t group = 32;
    const size_t np = (size_t)n_periods, nn = (size_t)n;
    if (!ctx->copy_stream) TLS_HIP(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    int rc = reserve_batch_staging(ctx, group, nn, 3 * (size_t)group * np);
    for (auto& sl : ctx->slot)
        if (rc || (rc = reserve_batch_slot(ctx, sl, group, nn, np))) return rc;
    TLS_HIP(ctx, ctx->d_perm.reserve(perm_scratch_words(ctx, nn)));
    const int64_t n_groups = (n_curves + group - 1) / group;
    auto drain = [&](int64_t g) -> int {   // results of group g: wait for its download, copy to the caller's arrays
        auto& sl = ctx->slot[g & 1];
        const int64_t c0 = g * group, gc = std::min(group, n_curves - c0);
        TLS_HIP(ctx, hipEventSynchronize(sl.ev_out));
        const size_t cnt = (size_t)gc * np;
        std::memcpy(out_chi2 + c0 * n_periods, sl.h_out, cnt * 8);
        std::memcpy(out_row + c0 * n_periods, sl.h_out + (size_t)group * np, cnt * 8);
        std::memcpy(out_depth + c0 * n_periods, sl.h_out + 2 * (size_t)group * np, cnt * 8);
        return TLS_OK;
    };
    ctx->batch_group_ms.assign((size_t)n_groups, 0.0);
    ctx->batch_group_wait_ms.clear();
    GroupState st;
    for (int64_t g = 0; g < n_groups; ++g) {
        auto& sl = ctx->slot[g & 1];
        const int64_t c0 = g * group, gc = std::min(group, n_curves - c0);
        const auto group_t0 = std::chrono::steady_clock::now();   // (pipelined: a group's time is its host loop pass, waits for older groups included)
        if (g >= 2 && (rc = drain(g - 2))) return rc;           // the slot's buffers are free again
        if ((rc = stage_group(ctx, sl, y, dy, n, c0, gc, group, st)) || (rc = upload_group(ctx, sl, st, nn, ctx->copy_stream))) return rc;
        TLS_HIP(ctx, hipEventRecord(sl.ev_in, ctx->copy_stream));
        TLS_HIP(ctx, hipStreamWaitEvent(main_stream(ctx), sl.ev_in, 0));
        if ((rc = search_group(ctx, sl, st))) return rc;
        TLS_HIP(ctx, hipEventRecord(sl.ev_kernel, main_stream(ctx)));
        TLS_HIP(ctx, hipStreamWaitEvent(ctx->copy_stream, sl.ev_kernel, 0));
        TLS_HIP(ctx, hipMemcpyAsync(sl.h_out, sl.d_chi2.ptr, (size_t)gc * np * 8, hipMemcpyDeviceToHost, ctx->copy_stream));
        TLS_HIP(ctx, hipMemcpyAsync(sl.h_out + (size_t)group * np, sl.d_row.ptr, (size_t)gc * np * 8, hipMemcpyDeviceToHost, ctx->copy_stream));
        TLS_HIP(ctx, hipMemcpyAsync(sl.h_out + 2 * (size_t)group * np, sl.d_depth.ptr, (size_t)gc * np * 8, hipMemcpyDeviceToHost, ctx->copy_stream));
        TLS_HIP(ctx, hipEventRecord(sl.ev_out, ctx->copy_stream));
        ctx->batch_group_ms[(size_t)g] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - group_t0).count();
    }
    for (int64_t g = std::max<int64_t>(0, n_groups - 2); g < n_groups; ++g)
        if ((rc = drain(g))) return rc;
    // the context keeps the plan, but the search ran on the batch slots: a staged execute
    // must be preceded by tls_update_flux or a new tls_prepare
    ctx->executed = false;
    return TLS_OK;
}

int tls_search_batch(tls_ctx* ctx, const double* t, const double* y, const double* dy, int64_t n, int64_t n_curves,
                     const double* periods, int64_t n_periods, const tls_template* tmpl, const tls_params* params,
                     double* out_chi2, int64_t* out_row, double* out_depth) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (n_curves < 0) return fail(ctx, TLS_E_ARG, "negative number of light curves");
    if (n_curves == 0) return TLS_OK;
    if (!y || !dy || !out_chi2 || !out_row || !out_depth) return fail(ctx, TLS_E_ARG, "null argument");
    int rc = tls_prepare(ctx, t, y, dy, n, periods, n_periods, tmpl, params);   // the plan, from the first curve
    if (rc) return rc;
    if (n_periods == 0) return TLS_OK;
    return end_batch(ctx, search_batch_impl(ctx, y, dy, n, n_curves, n_periods, out_chi2, out_row, out_depth));
}

static int power_batch_impl(tls_ctx* ctx, const double* t, const double* y, const double* dy, int64_t n, int64_t n_curves,
                            const double* periods, int64_t n_periods, const tls_template* tmpl, const tls_params* params,
                            int64_t median_kernel, tls_power_summary* out_summary, double* out_chi2, int64_t* out_row,
                            double* out_depth, double* out_power, double* out_SR, double* out_power_raw,
                            const StatsRequest* sr, const ModelsRequest* mr = nullptr, const PeaksRequest* pk = nullptr,
                            const PeakFitsRequest* pf = nullptr, const PhaseScanRequest* ps = nullptr);

int tls_power_batch(tls_ctx* ctx, const double* t, const double* y, const double* dy, int64_t n, int64_t n_curves,
                    const double* periods, int64_t n_periods, const tls_template* tmpl, const tls_params* params,
                    int64_t median_kernel, tls_power_summary* out_summary, double* out_chi2, int64_t* out_row,
                    double* out_depth, double* out_power, double* out_SR, double* out_power_raw) {
    return end_batch(ctx, power_batch_impl(ctx, t, y, dy, n, n_curves, periods, n_periods, tmpl, params, median_kernel,
                                           out_summary, out_chi2, out_row, out_depth, out_power, out_SR, out_power_raw, nullptr));
}

int tls_power_batch_stats(tls_ctx* ctx, const double* t, const double* y, const double* dy, int64_t n, int64_t n_curves,
                          const double* periods, int64_t n_periods, const tls_template* tmpl, const tls_params* params,
                          int64_t median_kernel, tls_power_summary* out_summary, double* out_chi2, int64_t* out_row,
                          double* out_depth, double* out_power, double* out_SR, double* out_power_raw,
                          const double* row_duration, double fill_factor, const double* root, const double* root_count,
                          int64_t n_root,
                          tls_transit_stats* out_stats, int64_t max_epochs, double* out_per_transit, int64_t* out_n_epochs) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (!t || !tmpl) return fail(ctx, TLS_E_ARG, "null argument");
    const StatsRequest sr = stats_request(row_duration, tmpl->n_rows, fill_factor, root, root_count, n_root, max_epochs, out_stats,
                                          out_per_transit, out_n_epochs);
    const int rc = check_stats_request(ctx, sr, t, n, tmpl->n_rows);
    if (rc) return rc;
    return end_batch(ctx, power_batch_impl(ctx, t, y, dy, n, n_curves, periods, n_periods, tmpl, params, median_kernel,
                                           out_summary, out_chi2, out_row, out_depth, out_power, out_SR, out_power_raw, &sr));
}

int tls_power_batch_models(tls_ctx* ctx, const double* t, const double* y, const double* dy, int64_t n, int64_t n_curves,
                           const double* periods, int64_t n_periods, const tls_template* tmpl, const tls_params* params,
                           int64_t median_kernel, tls_power_summary* out_summary, double* out_chi2, int64_t* out_row,
                           double* out_depth, double* out_power, double* out_SR, double* out_power_raw,
                           const double* row_duration, double fill_factor, const double* root, const double* root_count,
                           int64_t n_root,
                           tls_transit_stats* out_stats, int64_t max_epochs, double* out_per_transit, int64_t* out_n_epochs,
                           const double* curve_t, const double* curve_f, int64_t curve_n, double curve_lo, double curve_hi,
                           double maxw, int64_t lc_cap, double* out_folded, double* out_model_folded, double* out_lc,
                           int64_t* out_lc_len) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (!t || !tmpl) return fail(ctx, TLS_E_ARG, "null argument");
    const StatsRequest sr = stats_request(row_duration, tmpl->n_rows, fill_factor, root, root_count, n_root, max_epochs, out_stats,
                                          out_per_transit, out_n_epochs);
    const ModelsRequest mr = models_request(curve_t, curve_f, curve_n, curve_lo, curve_hi, maxw, lc_cap, out_folded,
                                            out_model_folded, out_lc, out_lc_len);
    int rc = check_stats_request(ctx, sr, t, n, tmpl->n_rows);
    if (rc || (rc = check_models_request(ctx, mr, n))) return rc;
    return end_batch(ctx, power_batch_impl(ctx, t, y, dy, n, n_curves, periods, n_periods, tmpl, params, median_kernel,
                                           out_summary, out_chi2, out_row, out_depth, out_power, out_SR, out_power_raw,
                                           &sr, &mr));
}

int tls_power_batch_peaks(tls_ctx* ctx, const double* t, const double* y, const double* dy, int64_t n, int64_t n_curves,
                          const double* periods, int64_t n_periods, const tls_template* tmpl, const tls_params* params,
                          int64_t median_kernel, tls_power_summary* out_summary, double* out_chi2, int64_t* out_row,
                          double* out_depth, double* out_power, double* out_SR, double* out_power_raw,
                          const double* row_duration, double fill_factor, const double* root, const double* root_count,
                          int64_t n_root,
                          tls_transit_stats* out_stats, int64_t max_epochs, double* out_per_transit, int64_t* out_n_epochs,
                          int64_t k, double min_separation, const double* ratios, int64_t n_ratios, double min_power,
                          tls_peak* out_peaks, int64_t* out_n_peaks) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (!t || !tmpl) return fail(ctx, TLS_E_ARG, "null argument");
    PeaksRequest pk;
    pk.k = k; pk.sep = min_separation; pk.ratios = ratios; pk.n_ratios = n_ratios; pk.min_power = min_power;
    pk.out = out_peaks; pk.out_n = out_n_peaks;
    int rc = check_peaks_request(ctx, pk, n_periods);
    if (rc) return rc;
    if (n_curves > 0 && (!out_peaks || !out_n_peaks)) return fail(ctx, TLS_E_ARG, "null peaks argument");
    StatsRequest sr;
    if (out_stats) {   // (no statistics wanted: their inputs are not read)
        sr = stats_request(row_duration, tmpl->n_rows, fill_factor, root, root_count, n_root, max_epochs, out_stats,
                           out_per_transit, out_n_epochs);
        if ((rc = check_stats_request(ctx, sr, t, n, tmpl->n_rows))) return rc;
    }
    return end_batch(ctx, power_batch_impl(ctx, t, y, dy, n, n_curves, periods, n_periods, tmpl, params, median_kernel,
                                           out_summary, out_chi2, out_row, out_depth, out_power, out_SR, out_power_raw,
                                           out_stats ? &sr : nullptr, nullptr, &pk));
}

int tls_power_batch_peak_fits(tls_ctx* ctx, const double* t, const double* y, const double* dy, int64_t n, int64_t n_curves,
                              const double* periods, int64_t n_periods, const tls_template* tmpl, const tls_params* params,
                              int64_t median_kernel, tls_power_summary* out_summary, double* out_chi2, int64_t* out_row,
                              double* out_depth, double* out_power, double* out_SR, double* out_power_raw,
                              const double* row_duration, double fill_factor, const double* root, const double* root_count,
                              int64_t n_root,
                              tls_transit_stats* out_stats, int64_t max_epochs, double* out_per_transit, int64_t* out_n_epochs,
                              int64_t k, double min_separation, const double* ratios, int64_t n_ratios, double min_power,
                              tls_peak* out_peaks, int64_t* out_n_peaks, tls_peak_fit* out_fits) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (!t || !tmpl) return fail(ctx, TLS_E_ARG, "null argument");
    PeaksRequest pk;
    pk.k = k; pk.sep = min_separation; pk.ratios = ratios; pk.n_ratios = n_ratios; pk.min_power = min_power;
    pk.out = out_peaks; pk.out_n = out_n_peaks;
    int rc = check_peaks_request(ctx, pk, n_periods);
    if (rc) return rc;
    if (n_curves > 0 && (!out_peaks || !out_n_peaks || !out_fits)) return fail(ctx, TLS_E_ARG, "null peaks argument");
    // (the fits read the statistics inputs whether or not the best pick's statistics are wanted)
    const StatsRequest sr = stats_request(row_duration, tmpl->n_rows, fill_factor, root, root_count, n_root, max_epochs, out_stats,
                                          out_stats ? out_per_transit : nullptr, out_stats ? out_n_epochs : nullptr);
    if ((rc = check_stats_request(ctx, sr, t, n, tmpl->n_rows, false))) return rc;
    PeakFitsRequest pf;
    pf.k = k; pf.inputs = &sr; pf.out = out_fits;
    return end_batch(ctx, power_batch_impl(ctx, t, y, dy, n, n_curves, periods, n_periods, tmpl, params, median_kernel,
                                           out_summary, out_chi2, out_row, out_depth, out_power, out_SR, out_power_raw,
                                           out_stats ? &sr : nullptr, nullptr, &pk, &pf));
}

int tls_power_batch_phase_scan(tls_ctx* ctx, const double* t, const double* y, const double* dy, int64_t n, int64_t n_curves,
                               const double* periods, int64_t n_periods, const tls_template* tmpl, const tls_params* params,
                               int64_t median_kernel, tls_power_summary* out_summary, double* out_chi2, int64_t* out_row,
                               double* out_depth, double* out_power, double* out_SR, double* out_power_raw,
                               const double* row_duration, double fill_factor, const double* root, const double* root_count,
                               int64_t n_root,
                               tls_transit_stats* out_stats, int64_t max_epochs, double* out_per_transit, int64_t* out_n_epochs,
                               int64_t k, double min_separation, const double* ratios, int64_t n_ratios, double min_power,
                               tls_peak* out_peaks, int64_t* out_n_peaks, tls_peak_fit* out_fits, int64_t max_bins,
                               int64_t min_count, tls_phase_record* out_scans) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (!t || !tmpl) return fail(ctx, TLS_E_ARG, "null argument");
    PeaksRequest pk;
    pk.k = k; pk.sep = min_separation; pk.ratios = ratios; pk.n_ratios = n_ratios; pk.min_power = min_power;
    pk.out = out_peaks; pk.out_n = out_n_peaks;
    int rc = check_peaks_request(ctx, pk, n_periods);
    if (rc) return rc;
    PhaseScanRequest ps;
    ps.max_bins = max_bins; ps.min_count = min_count; ps.out = out_scans;
    if ((rc = check_phase_scan_request(ctx, ps))) return rc;
    if (n_curves > 0 && (!out_peaks || !out_n_peaks || !out_fits || !out_scans)) return fail(ctx, TLS_E_ARG, "null peaks argument");
    const StatsRequest sr = stats_request(row_duration, tmpl->n_rows, fill_factor, root, root_count, n_root, max_epochs, out_stats,
                                          out_stats ? out_per_transit : nullptr, out_stats ? out_n_epochs : nullptr);
    if ((rc = check_stats_request(ctx, sr, t, n, tmpl->n_rows, false))) return rc;
    PeakFitsRequest pf;
    pf.k = k; pf.inputs = &sr; pf.out = out_fits;
    return end_batch(ctx, power_batch_impl(ctx, t, y, dy, n, n_curves, periods, n_periods, tmpl, params, median_kernel,
                                           out_summary, out_chi2, out_row, out_depth, out_power, out_SR, out_power_raw,
                                           out_stats ? &sr : nullptr, nullptr, &pk, &pf, &ps));
}

int tls_phase_scan(tls_ctx* ctx, const double* t, const double* y, int64_t n, int64_t n_curves, const int64_t* curve,
                   const double* period, const double* T0, const double* duration, int64_t n_fits, int64_t max_bins,
                   int64_t min_count, tls_phase_record* out) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    PhaseScanRequest ps;
    ps.max_bins = max_bins; ps.min_count = min_count; ps.out = out;
    int rc = check_phase_scan_request(ctx, ps);
    if (rc) return rc;
    if (n_fits < 0 || n_curves < 0) return fail(ctx, TLS_E_ARG, "phase scan: negative count");
    if (n_fits == 0) return TLS_OK;
    if (!t || !y || !curve || !period || !T0 || !duration || !out) return fail(ctx, TLS_E_ARG, "null argument");
    if ((rc = check_batch(ctx, "phase scan", n, INT32_MAX, "[1, 2^31)", n_fits, n_curves))) return rc;
    for (int64_t i = 0; i < n; ++i)       // (finite is all this entry asks of them: not check_time_stamps)
        if (!std::isfinite(t[i])) return fail(ctx, TLS_E_ARG, "phase scan: the time stamps must be finite");
    std::vector<int> h_curve((size_t)n_fits);
    for (int64_t f = 0; f < n_fits; ++f) {
        if (curve[f] < 0 || curve[f] >= n_curves) return fail(ctx, TLS_E_ARG, "phase scan: curve out of range [0, n_curves)");
        h_curve[(size_t)f] = (int)curve[f];
    }
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)n, rows = (size_t)n_curves, fits = (size_t)n_fits, words = (size_t)tlsdev::kPhaseWords;
    // (the whole batch at once: DESIGN.md "Phase scan")
    double *d_t, *d_y, *d_period, *d_T0, *d_duration, *d_out;
    int* d_curve;
    Arena L;
    L.add(d_t, nn);  L.add(d_y, rows * nn);  L.add(d_period, fits);  L.add(d_T0, fits);  L.add(d_duration, fits);
    L.add(d_out, words * fits);   // records
    L.add(d_curve, fits);         // curve of fit
    TLS_HIP(ctx, L.bind(ctx->d_scan));
    TLS_HIP(ctx, hipMemcpyAsync(d_t, t, nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_y, y, rows * nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_period, period, fits * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_T0, T0, fits * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_duration, duration, fits * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_curve, h_curve.data(), fits * sizeof(int), hipMemcpyHostToDevice, main_stream(ctx)));
    if ((rc = enqueue_phase_scan(ctx, ps, n_fits, d_t, d_y, n, d_curve, d_period, 1, d_T0, d_duration, 1, nullptr, d_out))) {
        (void)hipStreamSynchronize(main_stream(ctx));
        return rc;
    }
    ctx->last_kernel = "tls_phase_scan";
    TLS_HIP(ctx, hipMemcpyAsync(out, d_out, words * fits * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
    // (h_curve is read by the copy above until the stream is done)
    TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));
    return TLS_OK;
}

// ---- single-transit events (tls_single.hip.h, DESIGN.md "Single-transit events"): the statistic kernel over (tile, curve)
// and the selection kernel, one workgroup a curve, slab by slab; the planes stay in the context's scratch unless asked for
static_assert(sizeof(tls_single_event) == tlsdev::kSingleEventWords * 8, "tls_single_event is the kernel's record");
static_assert(TLS_SINGLE_MAX_WIDTH == tlsdev::kSingleMaxWidth && TLS_SINGLE_MAX_K == tlsdev::kSingleMaxK, "the header's limits");

int tls_single_transits(tls_ctx* ctx, const double* t, const double* y, const double* dy, int64_t n, int64_t n_curves,
                        const double* shape_values, const int64_t* shape_offset, const int64_t* width, const double* span_max,
                        int64_t n_rows, double depth_min, int64_t k, double min_ses, double separation,
                        tls_single_event* out_events, int64_t* out_n_events, double* out_ses, int64_t* out_row,
                        double* out_depth) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (n_curves < 0 || n_rows < 0 || n < 0) return fail(ctx, TLS_E_ARG, "single transits: negative count");
    if (k < 1 || k > TLS_SINGLE_MAX_K) return fail(ctx, TLS_E_ARG, "single transits: k out of range [1, 32]");
    if (!(std::isfinite(depth_min) && depth_min >= 0.0)) return fail(ctx, TLS_E_ARG, "single transits: depth_min must be finite and >= 0");
    if (!(std::isfinite(separation) && separation >= 0.0)) return fail(ctx, TLS_E_ARG, "single transits: separation must be finite and >= 0");
    if (std::isnan(min_ses)) return fail(ctx, TLS_E_ARG, "single transits: min_ses is NaN");
    RowTables tb;
    int rc = build_row_tables(ctx, "single transits", "null argument", shape_values, shape_offset, width, span_max, n_rows, false, tb);
    if (rc || n_curves == 0) return rc;
    if (!t || !y || !dy || !out_events || !out_n_events) return fail(ctx, TLS_E_ARG, "null argument");
    if (n < 1 || n > tlsdev::kSingleMaxPoints) return fail(ctx, TLS_E_ARG, "single transits: n out of range [1, 2^20]");
    if ((rc = check_time_stamps(ctx, "single transits", t, n))) return rc;
    const size_t n_taps = tb.n_taps;
    const int max_width = (int)width[n_rows - 1];
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)n, words = (size_t)k * tlsdev::kSingleEventWords;
    // curves per launch: at most 256 MB of rows and planes (as the detrending slabs), 36 bytes a point
    const int64_t slab = std::max<int64_t>(1, std::min<int64_t>({n_curves, (int64_t)65535, (int64_t)((256u << 20) / (36 * nn))}));
    const size_t sl = (size_t)slab;
    double *d_t, *d_taps, *d_y, *d_dy, *d_ses, *d_depth, *d_events;
    tlsdev::SingleRow* d_rows;
    long long* d_n_events;
    int* d_row;
    Arena L;
    L.add(d_t, nn);  L.add(d_rows, (size_t)n_rows);  L.add(d_taps, 2 * n_taps);
    L.add(d_y, sl * nn);          // of one slab, from here on
    L.add(d_dy, sl * nn);  L.add(d_ses, sl * nn);  L.add(d_depth, sl * nn);  L.add(d_events, sl * words);
    L.add(d_n_events, sl);  L.add(d_row, sl * nn);
    TLS_HIP(ctx, L.bind(ctx->d_single));
    if ((rc = ensure_check_counters(ctx))) return rc;
    tlsdev::SingleArgs a;
    a.t = d_t; a.y = d_y; a.dy = d_dy; a.rows = d_rows; a.taps = d_taps;
    a.ses = d_ses; a.row = d_row; a.depth = d_depth; a.check = ctx->d_check.ptr;
    a.depth_min = depth_min; a.n = (int)n; a.n_rows = (int)n_rows;
    a.halo_lo = (max_width - 1) / 2; a.halo_hi = max_width / 2;
    tlsdev::SingleSelectArgs s;
    s.t = d_t; s.ses = d_ses; s.row = d_row; s.depth = d_depth; s.rows = d_rows;
    s.events = d_events; s.n_events = d_n_events; s.check = ctx->d_check.ptr;
    s.min_ses = min_ses; s.separation = separation; s.n = (int)n; s.n_rows = (int)n_rows; s.k = (int)k;
    const size_t lds = tlsdev::single_lds_bytes(max_width), select_lds = tlsdev::single_select_lds_bytes((int)n);
    auto statistic = tlsdev::tls_single_statistic_kernel;
    auto select = tlsdev::tls_single_select_kernel;
    TLS_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(statistic), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    TLS_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(select), hipFuncAttributeMaxDynamicSharedMemorySize, (int)select_lds));
    TLS_HIP(ctx, hipMemcpyAsync(d_t, t, nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_rows, tb.rows.data(), (size_t)n_rows * sizeof(tlsdev::SingleRow), hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_taps, tb.taps.data(), 2 * n_taps * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    const unsigned tiles = (unsigned)((n + tlsdev::kSingleTile - 1) / tlsdev::kSingleTile);
    std::vector<int> h_row(out_row ? sl * nn : 0);
    for (int64_t k0 = 0; k0 < n_curves; k0 += slab) {
        const int64_t curves = std::min<int64_t>(slab, n_curves - k0);
        const size_t bytes = (size_t)curves * nn * 8, first = (size_t)k0 * nn;
        TLS_HIP(ctx, hipMemcpyAsync(d_y, y + first, bytes, hipMemcpyHostToDevice, main_stream(ctx)));
        TLS_HIP(ctx, hipMemcpyAsync(d_dy, dy + first, bytes, hipMemcpyHostToDevice, main_stream(ctx)));
        hipLaunchKernelGGL(statistic, dim3(tiles, (unsigned)curves), dim3(tlsdev::kSingleThreads), lds, main_stream(ctx), a);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) {
            hipLaunchKernelGGL(select, dim3((unsigned)curves), dim3(tlsdev::kSingleSelectThreads), select_lds, main_stream(ctx), s);
            e = hipGetLastError();
        }
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(main_stream(ctx));
            return fail(ctx, TLS_E_HIP, std::string("single transits launch: ") + hipGetErrorString(e));
        }
        ctx->last_kernel = "tls_single_transits";
        TLS_HIP(ctx, hipMemcpyAsync(out_events + (size_t)k0 * (size_t)k, d_events, (size_t)curves * words * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        TLS_HIP(ctx, hipMemcpyAsync(out_n_events + k0, d_n_events, (size_t)curves * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        if (out_ses) TLS_HIP(ctx, hipMemcpyAsync(out_ses + first, d_ses, bytes, hipMemcpyDeviceToHost, main_stream(ctx)));
        if (out_depth) TLS_HIP(ctx, hipMemcpyAsync(out_depth + first, d_depth, bytes, hipMemcpyDeviceToHost, main_stream(ctx)));
        if (out_row) TLS_HIP(ctx, hipMemcpyAsync(h_row.data(), d_row, (size_t)curves * nn * sizeof(int), hipMemcpyDeviceToHost, main_stream(ctx)));
        // (the next slab overwrites the device rows, and tb is read by the copies above until the stream is done)
        TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));
        if (out_row) for (size_t i = 0; i < (size_t)curves * nn; ++i) out_row[first + i] = h_row[i];
    }
    return TLS_OK;
}

// ---- transit times and the refitted ephemeris (tls_times.hip.h, DESIGN.md "Transit times"): the pairs kernel over the curves a
// slab of candidates reads, then one workgroup a candidate, slab by slab
static_assert(sizeof(tls_ephemeris) == tlsdev::kTimesEphemerisWords * 8, "tls_ephemeris is the kernel's record");
static_assert(sizeof(tls_transit_time) == tlsdev::kTimesTimeWords * 8, "tls_transit_time is the kernel's record");
static_assert(TLS_TIMES_MAX_REACH == tlsdev::kTimesMaxReach && TLS_TIMES_MAX_EPOCHS == tlsdev::kTimesMaxEpochs, "the header's limits");

int tls_transit_times(tls_ctx* ctx, const double* t, const double* y, const double* dy, int64_t n, int64_t n_curves,
                      const int64_t* curve, const double* period, const double* T0, const int64_t* row, const int64_t* reach,
                      int64_t n_fits, const double* shape_values, const int64_t* shape_offset, const int64_t* width,
                      const double* span_max, int64_t n_rows, double depth_min, double min_ses, int64_t max_epochs,
                      tls_ephemeris* out, tls_transit_time* out_times) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (n_fits < 0 || n_curves < 0 || n_rows < 0 || n < 0) return fail(ctx, TLS_E_ARG, "transit times: negative count");
    if (max_epochs < 1 || max_epochs > TLS_TIMES_MAX_EPOCHS) return fail(ctx, TLS_E_ARG, "transit times: max_epochs out of range [1, 65536]");
    if (!(std::isfinite(depth_min) && depth_min >= 0.0)) return fail(ctx, TLS_E_ARG, "transit times: depth_min must be finite and >= 0");
    if (std::isnan(min_ses)) return fail(ctx, TLS_E_ARG, "transit times: min_ses is NaN");
    if (n_fits == 0) return TLS_OK;
    RowTables tb;
    int rc = build_row_tables(ctx, "transit times", "null argument", shape_values, shape_offset, width, span_max, n_rows, true, tb);
    if (rc) return rc;
    if (!t || !y || !dy || !curve || !period || !T0 || !row || !reach || !out || !out_times) return fail(ctx, TLS_E_ARG, "null argument");
    if ((rc = check_batch(ctx, "transit times", n, tlsdev::kTimesMaxPoints, "[1, 2^30]", n_fits, n_curves))
        || (rc = check_time_stamps(ctx, "transit times", t, n)))
        return rc;
    if ((rc = check_curves(ctx, "transit times", curve, n_fits, n_curves, [&](int64_t f) {
            if (row[f] < 0 || row[f] >= n_rows) return fail(ctx, TLS_E_ARG, "transit times: row out of range [0, n_rows)");
            if (reach[f] < 1 || reach[f] > TLS_TIMES_MAX_REACH) return fail(ctx, TLS_E_ARG, "transit times: reach out of range [1, 4096]");
            return TLS_OK;
        })))
        return rc;
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)n, me = (size_t)max_epochs, n_taps = tb.n_taps;
    const size_t eph_words = tlsdev::kTimesEphemerisWords, time_words = (size_t)tlsdev::kTimesTimeWords * me;
    // a slab: at most 1024 candidates on at most 1024 curves, 256 MB of curves (32 bytes a point) and 256 MB of epoch records
    const size_t budget = 256u << 20;
    const size_t cs = std::max<size_t>(1, std::min<size_t>({(size_t)n_curves, 1024, budget / (32 * nn)}));
    const size_t sl = std::max<size_t>(1, std::min<size_t>({(size_t)n_fits, 1024, budget / (8 * time_words)}));
    double2* d_pairs;
    double *d_y, *d_dy, *d_out, *d_out_times, *d_period, *d_T0, *d_t, *d_taps, *d_slopes;
    int* d_ints;
    tlsdev::SingleRow* d_rows;
    Arena L;
    L.add(d_pairs, cs * nn);            // of one slab, down to the int columns
    L.add(d_y, cs * nn);  L.add(d_dy, cs * nn);  L.add(d_out, sl * eph_words);  L.add(d_out_times, sl * time_words);
    L.add(d_period, sl);  L.add(d_T0, sl);  L.add(d_ints, 3 * sl);   // slot | row | reach
    L.add(d_t, nn);                     // what every slab shares, from here on
    L.add(d_rows, (size_t)n_rows);  L.add(d_taps, 2 * n_taps);  L.add(d_slopes, 3 * n_taps);
    TLS_HIP(ctx, L.bind(ctx->d_times));
    if ((rc = ensure_check_counters(ctx))) return rc;
    tlsdev::TimesPairsArgs p;
    p.y = d_y; p.dy = d_dy; p.pairs = d_pairs;
    tlsdev::TimesArgs a;
    a.t = d_t; a.pairs = d_pairs; a.rows = d_rows; a.taps = d_taps; a.slopes = d_slopes;
    a.slot = d_ints; a.row = d_ints + sl; a.reach = d_ints + 2 * sl;
    a.period = d_period; a.T0 = d_T0; a.out = d_out; a.out_times = d_out_times; a.check = ctx->d_check.ptr;
    a.depth_min = depth_min; a.min_ses = min_ses; a.n = (int)n; a.max_epochs = (int)max_epochs;
    auto times_kernel = tlsdev::tls_transit_times_kernel;
    TLS_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(times_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     tlsdev::kTimesLdsUnits * 8));
    TLS_HIP(ctx, hipMemcpyAsync(d_t, t, nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_rows, tb.rows.data(), (size_t)n_rows * sizeof(tlsdev::SingleRow), hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_taps, tb.taps.data(), 2 * n_taps * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_slopes, tb.slopes.data(), 3 * n_taps * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    const SlabStage stage{"transit times", "tls_transit_times", curve, n_fits, nn, cs, sl,
                          {{d_y, y}, {d_dy, dy}}, {{d_period, period}, {d_T0, T0}}, d_ints, 3};
    return run_candidate_slabs(ctx, stage,
        [&](int64_t f, int* at) {
            at[sl] = (int)row[f];
            at[2 * sl] = (int)reach[f];
            return tlsdev::times_lds_bytes((int)reach[f], (int)max_epochs);
        },
        [&](const SlabView& s) {
            if (launch_times_pairs(ctx, p, s.curves, nn))
                hipLaunchKernelGGL(times_kernel, dim3((unsigned)s.fits), dim3(tlsdev::kTimesThreads), s.lds, main_stream(ctx), a);
        },
        [&](const SlabView& s) {
            TLS_HIP(ctx, hipMemcpyAsync(out + s.f0, d_out, s.fits * eph_words * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
            TLS_HIP(ctx, hipMemcpyAsync(out_times + (size_t)s.f0 * me, d_out_times, s.fits * time_words * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
            return TLS_OK;
        });
}

// ---- period aliases of event pairs (tls_aliases.hip.h, DESIGN.md "Event periods"): the pairs kernel of the transit times over
// the curves a slab of event pairs reads, the (N, D) plane of every (curve, row) group of the slab, then one workgroup an
// event pair, slab by slab
static_assert(sizeof(tls_event_pair) == tlsdev::kAliasPairWords * 8, "tls_event_pair is the kernel's record");
static_assert(sizeof(tls_event_alias) == tlsdev::kAliasWords * 8, "tls_event_alias is the kernel's record");
static_assert(TLS_ALIAS_MAX == tlsdev::kAliasMax, "the header's limit");

int tls_event_periods(tls_ctx* ctx, const double* t, const double* y, const double* dy, int64_t n, int64_t n_curves,
                      const int64_t* curve, const int64_t* index_a, const int64_t* index_b, const int64_t* row,
                      const int64_t* reach, const double* offset, int64_t n_pairs, const double* shape_values,
                      const int64_t* shape_offset, const int64_t* width, const double* span_max, int64_t n_rows,
                      double period_min, int64_t max_aliases, double min_ses, double veto_sigma, tls_event_pair* out,
                      tls_event_alias* out_aliases) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    const std::string what = "event periods";
    if (n_pairs < 0 || n_curves < 0 || n_rows < 0 || n < 0) return fail(ctx, TLS_E_ARG, what + ": negative count");
    if (max_aliases < 1 || max_aliases > TLS_ALIAS_MAX) return fail(ctx, TLS_E_ARG, what + ": max_aliases out of range [1, 4096]");
    if (!(std::isfinite(period_min) && period_min > 0.0)) return fail(ctx, TLS_E_ARG, what + ": period_min must be finite and > 0");
    if (std::isnan(min_ses) || std::isnan(veto_sigma)) return fail(ctx, TLS_E_ARG, what + ": min_ses or veto_sigma is NaN");
    if (n_pairs == 0) return TLS_OK;
    RowTables tb;
    int rc = build_row_tables(ctx, what, "null argument", shape_values, shape_offset, width, span_max, n_rows, false, tb);
    if (rc) return rc;
    if (!t || !y || !dy || !curve || !index_a || !index_b || !row || !reach || !offset || !out) return fail(ctx, TLS_E_ARG, "null argument");
    if ((rc = check_batch(ctx, what, n, tlsdev::kAliasMaxPoints, "[1, 2^20]", n_pairs, n_curves)) || (rc = check_time_stamps(ctx, what, t, n)))
        return rc;
    if (!((t[n - 1] - t[0]) / period_min + 2.0 <= (double)TLS_TIMES_MAX_EPOCHS))
        return fail(ctx, TLS_E_ARG, what + ": period_min gives an alias more than 65536 epochs");
    int max_width = 0;
    if ((rc = check_curves(ctx, what, curve, n_pairs, n_curves, [&](int64_t f) {
            if (row[f] < 0 || row[f] >= n_rows) return fail(ctx, TLS_E_ARG, what + ": row out of range [0, n_rows)");
            if (reach[f] < 1 || reach[f] > TLS_TIMES_MAX_REACH) return fail(ctx, TLS_E_ARG, what + ": reach out of range [1, 4096]");
            if (index_a[f] < 0 || index_b[f] >= n || index_a[f] >= index_b[f])
                return fail(ctx, TLS_E_ARG, what + ": the event indices must be 0 <= index_a < index_b < n");
            if (!(std::isfinite(offset[f]) && offset[f] >= 0.0)) return fail(ctx, TLS_E_ARG, what + ": offset must be finite and >= 0");
            max_width = std::max(max_width, (int)width[row[f]]);
            return TLS_OK;
        })))
        return rc;
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)n, ma = (size_t)max_aliases, n_taps = tb.n_taps;
    const size_t pair_words = tlsdev::kAliasPairWords, alias_words = out_aliases ? (size_t)tlsdev::kAliasWords * ma : 0;
    // a slab: at most 1024 pairs on at most 1024 curves; 256 MB of curves (32 bytes a point), of planes (16 bytes a point and
    // group, a group an event pair at most) and of alias records
    const size_t budget = 256u << 20;
    const size_t cs = std::max<size_t>(1, std::min<size_t>({(size_t)n_curves, 1024, budget / (32 * nn)}));
    const size_t sl = std::max<size_t>(1, std::min<size_t>({(size_t)n_pairs, 1024, budget / (16 * nn), budget / (64 * ma)}));
    double2 *d_pairs, *d_plane;
    double *d_y, *d_dy, *d_out, *d_out_aliases, *d_offset, *d_t, *d_taps;
    int *d_ints, *d_groups;
    tlsdev::SingleRow* d_rows;
    Arena L;
    L.add(d_pairs, cs * nn);            // of one slab, down to the group columns
    L.add(d_plane, sl * nn);
    L.add(d_y, cs * nn);  L.add(d_dy, cs * nn);  L.add(d_out, sl * pair_words);  L.add(d_out_aliases, sl * alias_words);
    L.add(d_offset, sl);  L.add(d_ints, 5 * sl);     // slot | row | reach | index_a | index_b
    L.add(d_groups, 3 * sl);                         // every pair's group | every group's slot | every group's row
    L.add(d_t, nn);                     // what every slab shares, from here on
    L.add(d_rows, (size_t)n_rows);  L.add(d_taps, 2 * n_taps);
    TLS_HIP(ctx, L.bind(ctx->d_aliases));
    if ((rc = ensure_check_counters(ctx))) return rc;
    tlsdev::TimesPairsArgs p;
    p.y = d_y; p.dy = d_dy; p.pairs = d_pairs;
    tlsdev::AliasPlaneArgs pl;
    pl.t = d_t; pl.pairs = d_pairs; pl.rows = d_rows; pl.taps = d_taps; pl.group_slot = d_groups + sl; pl.group_row = d_groups + 2 * sl;
    pl.plane = d_plane; pl.check = ctx->d_check.ptr; pl.n = (int)n;
    tlsdev::AliasArgs a;
    a.t = d_t; a.plane = d_plane; a.group = d_groups; a.reach = d_ints + 2 * sl; a.index_a = d_ints + 3 * sl; a.index_b = d_ints + 4 * sl;
    a.offset = d_offset; a.out = d_out; a.out_aliases = d_out_aliases; a.check = ctx->d_check.ptr;
    a.period_min = period_min; a.min_ses = min_ses; a.veto_sigma = veto_sigma; a.n = (int)n; a.max_aliases = (int)max_aliases;
    const size_t plane_lds = tlsdev::alias_plane_lds_bytes(max_width), alias_lds = tlsdev::alias_lds_bytes((int)n);
    auto plane_kernel = tlsdev::tls_alias_plane_kernel;
    auto alias_kernel = alias_lds ? tlsdev::tls_event_aliases_kernel<true> : tlsdev::tls_event_aliases_kernel<false>;
    TLS_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(plane_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)plane_lds));
    if (alias_lds)
        TLS_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(alias_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         tlsdev::kAliasLdsPoints * 24));
    TLS_HIP(ctx, hipMemcpyAsync(d_t, t, nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_rows, tb.rows.data(), (size_t)n_rows * sizeof(tlsdev::SingleRow), hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_taps, tb.taps.data(), 2 * n_taps * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    const unsigned tiles = (unsigned)((nn + tlsdev::kAliasTile - 1) / tlsdev::kAliasTile);
    // the (slot, row) groups of a slab: its pairs in a stable sort by (slot, row), a new group where either changes
    std::vector<int> h_slot(sl), h_groups(3 * sl), order(sl);
    tlsslab::Slab again;
    const SlabStage stage{"event periods", "tls_event_periods", curve, n_pairs, nn, cs, sl,
                          {{d_y, y}, {d_dy, dy}}, {{d_offset, offset}}, d_ints, 5};
    return run_candidate_slabs(ctx, stage,
        [&](int64_t f, int* at) {
            at[sl] = (int)row[f];
            at[2 * sl] = (int)reach[f];
            at[3 * sl] = (int)index_a[f];
            at[4 * sl] = (int)index_b[f];
            return (size_t)0;
        },
        [&](const SlabView& s) {
            tlsslab::next_slab(curve, n_pairs, s.f0, cs, sl, h_slot.data(), again);   // (the slab's slots once more)
            for (size_t i = 0; i < s.fits; ++i) order[i] = (int)i;
            std::stable_sort(order.begin(), order.begin() + (ptrdiff_t)s.fits, [&](int u, int v) {
                const int64_t ru = row[s.f0 + u], rv = row[s.f0 + v];
                return h_slot[(size_t)u] != h_slot[(size_t)v] ? h_slot[(size_t)u] < h_slot[(size_t)v] : ru < rv;
            });
            size_t groups = 0;
            for (size_t k = 0; k < s.fits; ++k) {
                const int i = order[k];
                const int r = (int)row[s.f0 + i];
                if (k == 0 || h_groups[sl + groups - 1] != h_slot[(size_t)i] || h_groups[2 * sl + groups - 1] != r) {
                    h_groups[sl + groups] = h_slot[(size_t)i];
                    h_groups[2 * sl + groups] = r;
                    ++groups;
                }
                h_groups[(size_t)i] = (int)groups - 1;
            }
            if (hipMemcpyAsync(d_groups, h_groups.data(), 3 * sl * sizeof(int), hipMemcpyHostToDevice, main_stream(ctx)) != hipSuccess) return;
            if (!launch_times_pairs(ctx, p, s.curves, nn)) return;
            hipLaunchKernelGGL(plane_kernel, dim3(tiles, (unsigned)groups), dim3(tlsdev::kAliasThreads), plane_lds, main_stream(ctx), pl);
            if (hipPeekAtLastError() != hipSuccess) return;
            hipLaunchKernelGGL(alias_kernel, dim3((unsigned)s.fits), dim3(tlsdev::kAliasThreads), alias_lds, main_stream(ctx), a);
        },
        [&](const SlabView& s) {
            TLS_HIP(ctx, hipMemcpyAsync(out + s.f0, d_out, s.fits * pair_words * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
            if (out_aliases)
                TLS_HIP(ctx, hipMemcpyAsync(out_aliases + (size_t)s.f0 * ma, d_out_aliases, s.fits * alias_words * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
            return TLS_OK;
        });
}

// ---- per-transit event vetting (tls_events.hip.h, DESIGN.md "Event vetting"): the pairs kernel of the transit times over the
// curves a slab of candidates reads, then one workgroup a candidate, slab by slab
static_assert(sizeof(tls_event_summary) == tlsdev::kEventsSummaryWords * 8, "tls_event_summary is the kernel's record");
static_assert(sizeof(tls_event_record) == tlsdev::kEventsRecordWords * 8, "tls_event_record is the kernel's record");
static_assert(TLS_EVENTS_MAX_CHASE == tlsdev::kEventsMaxChase, "the header's limit");

int tls_event_vetting(tls_ctx* ctx, const double* t, const double* y, const double* dy, int64_t n, int64_t n_curves,
                      const int64_t* curve, const double* period, const double* T0, const int64_t* row, const int64_t* reach,
                      const int64_t* chase_reach, const int64_t* guard, const double* chase_span, int64_t n_fits,
                      const double* shape_values, const int64_t* shape_offset, const int64_t* width, const double* span_max,
                      int64_t n_rows, double depth_min, double min_ses, double chase_fraction, double chase_min,
                      double point_fraction, double step_fraction, int64_t max_epochs,
                      tls_event_summary* out, tls_event_record* out_events) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (n_fits < 0 || n_curves < 0 || n_rows < 0 || n < 0) return fail(ctx, TLS_E_ARG, "event vetting: negative count");
    if (max_epochs < 1 || max_epochs > TLS_TIMES_MAX_EPOCHS) return fail(ctx, TLS_E_ARG, "event vetting: max_epochs out of range [1, 65536]");
    if (!(std::isfinite(depth_min) && depth_min >= 0.0)) return fail(ctx, TLS_E_ARG, "event vetting: depth_min must be finite and >= 0");
    if (std::isnan(min_ses)) return fail(ctx, TLS_E_ARG, "event vetting: min_ses is NaN");
    if (!(chase_fraction > 0.0 && chase_fraction <= 1.0)) return fail(ctx, TLS_E_ARG, "event vetting: chase_fraction out of range (0, 1]");
    if (!(chase_min >= 0.0 && chase_min <= 1.0)) return fail(ctx, TLS_E_ARG, "event vetting: chase_min out of range [0, 1]");
    if (!(point_fraction > 0.0)) return fail(ctx, TLS_E_ARG, "event vetting: point_fraction must be > 0");
    if (!(step_fraction > 0.0)) return fail(ctx, TLS_E_ARG, "event vetting: step_fraction must be > 0");
    if (n_fits == 0) return TLS_OK;
    RowTables tb;
    int rc = build_row_tables(ctx, "event vetting", "event vetting: null argument", shape_values, shape_offset, width, span_max,
                              n_rows, false, tb);
    if (rc) return rc;
    if (!t || !y || !dy || !curve || !period || !T0 || !row || !reach || !chase_reach || !guard || !chase_span || !out || !out_events)
        return fail(ctx, TLS_E_ARG, "event vetting: null argument");
    if ((rc = check_batch(ctx, "event vetting", n, tlsdev::kTimesMaxPoints, "[1, 2^30]", n_fits, n_curves))
        || (rc = check_time_stamps(ctx, "event vetting", t, n)))
        return rc;
    if ((rc = check_curves(ctx, "event vetting", curve, n_fits, n_curves, [&](int64_t f) {
            if (row[f] < 0 || row[f] >= n_rows) return fail(ctx, TLS_E_ARG, "event vetting: row out of range [0, n_rows)");
            if (reach[f] < 1 || reach[f] > TLS_TIMES_MAX_REACH) return fail(ctx, TLS_E_ARG, "event vetting: reach out of range [1, 4096]");
            if (chase_reach[f] < 0 || chase_reach[f] > TLS_EVENTS_MAX_CHASE)
                return fail(ctx, TLS_E_ARG, "event vetting: chase_reach out of range [0, 8192]");
            if (guard[f] < 0) return fail(ctx, TLS_E_ARG, "event vetting: negative guard");
            if (!(std::isfinite(chase_span[f]) && chase_span[f] > 0.0))
                return fail(ctx, TLS_E_ARG, "event vetting: chase_span must be finite and > 0");
            return TLS_OK;
        })))
        return rc;
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)n, me = (size_t)max_epochs, n_taps = tb.n_taps;
    const size_t sum_words = tlsdev::kEventsSummaryWords, event_words = (size_t)tlsdev::kEventsRecordWords * me;
    // a slab: at most 1024 candidates on at most 1024 curves, 256 MB of curves (32 bytes a point) and 256 MB of event records
    // and held sums (16 doubles an epoch)
    const size_t budget = 256u << 20;
    const size_t cs = std::max<size_t>(1, std::min<size_t>({(size_t)n_curves, 1024, budget / (32 * nn)}));
    const size_t sl = std::max<size_t>(1, std::min<size_t>({(size_t)n_fits, 1024, budget / (8 * (event_words + 2 * me))}));
    double2 *d_pairs, *d_held;
    double *d_y, *d_dy, *d_out, *d_out_events, *d_period, *d_T0, *d_span, *d_t, *d_taps;
    int* d_ints;
    tlsdev::SingleRow* d_rows;
    Arena L;
    L.add(d_pairs, cs * nn);            // of one slab, down to the int columns
    L.add(d_held, sl * me);             // held (N, D)
    L.add(d_y, cs * nn);  L.add(d_dy, cs * nn);  L.add(d_out, sl * sum_words);  L.add(d_out_events, sl * event_words);
    L.add(d_period, sl);  L.add(d_T0, sl);  L.add(d_span, sl);
    L.add(d_ints, 5 * sl);              // slot | row | reach | chase | guard
    L.add(d_t, nn);                     // what every slab shares, from here on
    L.add(d_rows, (size_t)n_rows);  L.add(d_taps, 2 * n_taps);
    TLS_HIP(ctx, L.bind(ctx->d_vetting));
    if ((rc = ensure_check_counters(ctx))) return rc;
    tlsdev::TimesPairsArgs p;
    p.y = d_y; p.dy = d_dy; p.pairs = d_pairs;
    tlsdev::EventsArgs a;
    a.t = d_t; a.pairs = d_pairs; a.rows = d_rows; a.taps = d_taps;
    a.slot = d_ints; a.row = d_ints + sl; a.reach = d_ints + 2 * sl; a.chase = d_ints + 3 * sl; a.guard = d_ints + 4 * sl;
    a.period = d_period; a.T0 = d_T0; a.chase_span = d_span; a.out = d_out; a.out_events = d_out_events; a.held = d_held;
    a.check = ctx->d_check.ptr;
    a.depth_min = depth_min; a.min_ses = min_ses; a.chase_fraction = chase_fraction; a.chase_min = chase_min;
    a.point_fraction = point_fraction; a.step_fraction = step_fraction; a.n = (int)n; a.max_epochs = (int)max_epochs;
    auto events_kernel = tlsdev::tls_event_vetting_kernel;
    TLS_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(events_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     tlsdev::kTimesLdsUnits * 8));
    TLS_HIP(ctx, hipMemcpyAsync(d_t, t, nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_rows, tb.rows.data(), (size_t)n_rows * sizeof(tlsdev::SingleRow), hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_taps, tb.taps.data(), 2 * n_taps * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    const SlabStage stage{"event vetting", "tls_event_vetting", curve, n_fits, nn, cs, sl,
                          {{d_y, y}, {d_dy, dy}}, {{d_period, period}, {d_T0, T0}, {d_span, chase_span}}, d_ints, 5};
    return run_candidate_slabs(ctx, stage,
        [&](int64_t f, int* at) {
            at[sl] = (int)row[f];
            at[2 * sl] = (int)reach[f];
            at[3 * sl] = (int)chase_reach[f];
            at[4 * sl] = (int)std::min(guard[f], chase_reach[f]);   // (a guard at or beyond the reach: no chase window)
            return tlsdev::times_lds_bytes((int)reach[f], (int)max_epochs);
        },
        [&](const SlabView& s) {
            if (launch_times_pairs(ctx, p, s.curves, nn))
                hipLaunchKernelGGL(events_kernel, dim3((unsigned)s.fits), dim3(tlsdev::kEventsThreads), s.lds, main_stream(ctx), a);
        },
        [&](const SlabView& s) {
            TLS_HIP(ctx, hipMemcpyAsync(out + s.f0, d_out, s.fits * sum_words * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
            TLS_HIP(ctx, hipMemcpyAsync(out_events + (size_t)s.f0 * me, d_out_events, s.fits * event_words * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
            return TLS_OK;
        });
}

// ---- the trapezoid shape fit (tls_shape.hip.h, DESIGN.md "Shape fit"): the pairs kernel of the transit times over the curves
// a slab of candidates reads, then one workgroup a candidate, slab by slab
static_assert(sizeof(tls_shape_record) == tlsdev::kShapeWords * 8, "tls_shape_record is the kernel's record");
static_assert(TLS_SHAPE_MAX_UNITS == tlsdev::kShapeMaxUnits, "the header's limit");

int tls_shape_fit(tls_ctx* ctx, const double* t, const double* y, const double* dy, int64_t n, int64_t n_curves,
                  const double* period, const double* T0, const double* duration, const int64_t* curve, int64_t n_fits,
                  const double* ratio, int64_t nT, const double* ingress, int64_t nQ, const double* shift, int64_t nS,
                  double window, int64_t min_count, double depth_min, tls_shape_record* out) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (n_fits < 0 || n_curves < 0 || n < 0) return fail(ctx, TLS_E_ARG, "shape fit: negative count");
    if (nT < 1 || nQ < 1 || nS < 1) return fail(ctx, TLS_E_ARG, "shape fit: every table needs an entry");
    if (nT > TLS_SHAPE_MAX_UNITS || nQ > TLS_SHAPE_MAX_UNITS || nS > TLS_SHAPE_MAX_UNITS || nT * nQ * nS > TLS_SHAPE_MAX_UNITS)
        return fail(ctx, TLS_E_ARG, "shape fit: more than 65536 units");
    if (!ratio || !ingress || !shift) return fail(ctx, TLS_E_ARG, "null argument");
    for (const auto& table : {std::make_pair(ratio, nT), std::make_pair(ingress, nQ), std::make_pair(shift, nS)})
        for (int64_t i = 0; i < table.second; ++i)
            if (!std::isfinite(table.first[i]) || (i > 0 && table.first[i] < table.first[i - 1]))
                return fail(ctx, TLS_E_ARG, "shape fit: the tables must be finite and non-decreasing");
    if (!(ratio[0] > 0.0)) return fail(ctx, TLS_E_ARG, "shape fit: every ratio must be > 0");
    if (ingress[0] != 0.0 || ingress[nQ - 1] != 0.5) return fail(ctx, TLS_E_ARG, "shape fit: ingress must run from 0.0 to 0.5");
    if (!(std::isfinite(window) && window >= 0.5 * ratio[nT - 1] + std::max(std::fabs(shift[0]), std::fabs(shift[nS - 1]))))
        return fail(ctx, TLS_E_ARG, "shape fit: the window must be finite and hold the widest, farthest shifted model");
    if (min_count < 1) return fail(ctx, TLS_E_ARG, "shape fit: min_count < 1");
    if (!(std::isfinite(depth_min) && depth_min >= 0.0)) return fail(ctx, TLS_E_ARG, "shape fit: depth_min must be finite and >= 0");
    if (n_fits == 0) return TLS_OK;
    if (!t || !y || !dy || !curve || !period || !T0 || !duration || !out) return fail(ctx, TLS_E_ARG, "null argument");
    int rc;
    if ((rc = check_batch(ctx, "shape fit", n, tlsdev::kShapeMaxPoints, "[1, 2^22]", n_fits, n_curves))
        || (rc = check_time_stamps(ctx, "shape fit", t, n)) || (rc = check_curves(ctx, "shape fit", curve, n_fits, n_curves)))
        return rc;
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)n, words = tlsdev::kShapeWords;
    // a slab: at most 1024 candidates on at most 1024 curves, 256 MB of curves (32 bytes a point); the workgroups of a launch:
    // at most 1024, 256 MB of member scratch (24 bytes a point each)
    const size_t budget = 256u << 20;
    const size_t cs = std::max<size_t>(1, std::min<size_t>({(size_t)n_curves, 1024, budget / (32 * nn)}));
    const size_t sl = std::min<size_t>((size_t)n_fits, 1024);
    const size_t groups = std::max<size_t>(1, std::min<size_t>({sl, (size_t)tlsdev::kShapeMaxGroups, budget / (24 * nn)}));
    double2* d_pairs;
    double *d_y, *d_dy, *d_out, *d_period, *d_T0, *d_duration, *d_t, *d_ratio, *d_ingress, *d_shift, *d_scratch;
    int* d_slot;
    Arena L;
    L.add(d_pairs, cs * nn);            // of one slab, down to the slots
    L.add(d_y, cs * nn);  L.add(d_dy, cs * nn);  L.add(d_out, sl * words);  L.add(d_period, sl);  L.add(d_T0, sl);
    L.add(d_duration, sl);  L.add(d_slot, sl);
    L.add(d_t, nn);                     // what every slab shares, from here on
    L.add(d_ratio, (size_t)nT);  L.add(d_ingress, (size_t)nQ);  L.add(d_shift, (size_t)nS);  L.add(d_scratch, 3 * groups * nn);
    TLS_HIP(ctx, L.bind(ctx->d_shape));
    if ((rc = ensure_check_counters(ctx))) return rc;
    tlsdev::TimesPairsArgs p;
    p.y = d_y; p.dy = d_dy; p.pairs = d_pairs;
    tlsdev::ShapeArgs a;
    a.t = d_t; a.pairs = d_pairs; a.slot = d_slot; a.period = d_period; a.T0 = d_T0; a.duration = d_duration;
    a.ratio = d_ratio; a.ingress = d_ingress; a.shift = d_shift; a.scratch = d_scratch; a.out = d_out;
    a.check = ctx->d_check.ptr; a.window = window; a.depth_min = depth_min;
    a.n = (int)n; a.nT = (int)nT; a.nQ = (int)nQ; a.nS = (int)nS;
    a.min_count = (int)std::min<int64_t>(min_count, INT32_MAX);
    TLS_HIP(ctx, hipMemcpyAsync(d_t, t, nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_ratio, ratio, (size_t)nT * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_ingress, ingress, (size_t)nQ * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_shift, shift, (size_t)nS * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    const SlabStage stage{"shape fit", "tls_shape_fit", curve, n_fits, nn, cs, sl,
                          {{d_y, y}, {d_dy, dy}}, {{d_period, period}, {d_T0, T0}, {d_duration, duration}}, d_slot, 1};
    return run_candidate_slabs(ctx, stage, no_int_columns,
        [&](const SlabView& s) {
            a.fits = (int)s.fits;
            if (launch_times_pairs(ctx, p, s.curves, nn))
                hipLaunchKernelGGL(tlsdev::tls_shape_fit_kernel, dim3((unsigned)std::min(s.fits, groups)), dim3(tlsdev::kShapeThreads), 0, main_stream(ctx), a);
        },
        [&](const SlabView& s) {
            TLS_HIP(ctx, hipMemcpyAsync(out + s.f0, d_out, s.fits * words * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
            return TLS_OK;
        });
}

// ---- the limb-darkened transit fit (tls_transit_fit.hip.h, DESIGN.md "Transit fit"): the pairs kernel of the transit times
// over the curves a slab of candidates reads, then one workgroup a candidate, slab by slab
static_assert(sizeof(tls_transit_fit_record) == tlsdev::kTransitWords * 8, "tls_transit_fit_record is the kernel's record");
static_assert(TLS_TRANSIT_FIT_MAX_UNITS == tlsdev::kTransitMaxUnits && TLS_TRANSIT_FIT_MAX_M == tlsdev::kTransitMaxM
              && TLS_TRANSIT_FIT_MAX_SUB == tlsdev::kTransitMaxSub && TLS_TRANSIT_FIT_MAX_ROWS == tlsdev::kTransitMaxRows,
              "the header's limits");

int tls_transit_fit(tls_ctx* ctx, const double* t, const double* y, const double* dy, int64_t n, int64_t n_curves,
                    const int64_t* curve, const double* period, const double* T0, const double* duration,
                    const int64_t* row_first, int64_t n_fits, const double* k_rows, const double* profile, int64_t n_k,
                    int64_t M, const double* impact, int64_t n_b, const double* ratio, int64_t n_t, const double* shift,
                    int64_t n_s, const double* sub, int64_t n_sub, double window, int64_t min_count, double delta,
                    tls_transit_fit_record* out_records) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    const std::string what = "transit fit";
    if (n_fits < 0 || n_curves < 0 || n < 0) return fail(ctx, TLS_E_ARG, what + ": negative count");
    if (n_k < 1 || n_b < 1 || n_t < 1 || n_s < 1) return fail(ctx, TLS_E_ARG, what + ": every table needs an entry");
    if (n_k > TLS_TRANSIT_FIT_MAX_ROWS) return fail(ctx, TLS_E_ARG, what + ": more than 4096 profile rows");
    if (M < 1 || M > TLS_TRANSIT_FIT_MAX_M) return fail(ctx, TLS_E_ARG, what + ": M out of range [1, 4096]");
    if (n_sub < 1 || n_sub > TLS_TRANSIT_FIT_MAX_SUB) return fail(ctx, TLS_E_ARG, what + ": n_sub out of range [1, 16]");
    if (n_b > TLS_TRANSIT_FIT_MAX_UNITS || n_t > TLS_TRANSIT_FIT_MAX_UNITS || n_s > TLS_TRANSIT_FIT_MAX_UNITS
        || n_b * n_t * n_s > TLS_TRANSIT_FIT_MAX_UNITS)
        return fail(ctx, TLS_E_ARG, what + ": more than 65536 units");
    if (!k_rows || !profile || !impact || !ratio || !shift || !sub) return fail(ctx, TLS_E_ARG, what + ": null argument");
    for (const auto& table : {std::make_pair(k_rows, n_k), std::make_pair(impact, n_b), std::make_pair(ratio, n_t), std::make_pair(shift, n_s)})
        for (int64_t i = 0; i < table.second; ++i)
            if (!std::isfinite(table.first[i]) || (i > 0 && table.first[i] < table.first[i - 1]))
                return fail(ctx, TLS_E_ARG, what + ": the tables must be finite and non-decreasing");
    if (!(k_rows[0] > 0.0)) return fail(ctx, TLS_E_ARG, what + ": every k_rows must be > 0");
    if (!(impact[0] >= 0.0 && impact[n_b - 1] < 1.0)) return fail(ctx, TLS_E_ARG, what + ": every impact must be in [0, 1)");
    if (!(ratio[0] > 0.0)) return fail(ctx, TLS_E_ARG, what + ": every ratio must be > 0");
    double sub_reach = 0.0;
    for (int64_t s = 0; s < n_sub; ++s) {
        if (!std::isfinite(sub[s])) return fail(ctx, TLS_E_ARG, what + ": sub must be finite");
        sub_reach = std::max(sub_reach, std::fabs(sub[s]));
    }
    for (int64_t i = 0; i < n_k * (M + 1); ++i)
        if (!std::isfinite(profile[i])) return fail(ctx, TLS_E_ARG, what + ": the profile must be finite");
    const double reach = 0.5 * ratio[n_t - 1] + std::max(std::fabs(shift[0]), std::fabs(shift[n_s - 1]));
    if (!(std::isfinite(window) && window >= reach))
        return fail(ctx, TLS_E_ARG, what + ": the window must be finite and hold the widest, farthest shifted model");
    if (min_count < 1) return fail(ctx, TLS_E_ARG, what + ": min_count < 1");
    if (!(std::isfinite(delta) && delta >= 0.0)) return fail(ctx, TLS_E_ARG, what + ": delta must be finite and >= 0");
    if (n_fits == 0) return TLS_OK;
    if (!t || !y || !dy || !period || !T0 || !duration || !row_first || !out_records) return fail(ctx, TLS_E_ARG, what + ": null argument");
    int rc;
    if ((rc = check_batch(ctx, what, n, tlsdev::kShapeMaxPoints, "[1, 2^22]", n_fits, n_curves))
        || (rc = check_time_stamps(ctx, what, t, n))
        || (rc = check_curves(ctx, what, curve, n_fits, n_curves, [&](int64_t f) {
               if (row_first[f] < 0 || row_first[f] >= n_k) return fail(ctx, TLS_E_ARG, what + ": row_first out of range [0, n_k)");
               const double d = duration[f];
               if (std::isfinite(d) && d > 0.0 && !(window * d >= reach * d + sub_reach))
                   return fail(ctx, TLS_E_ARG, what + ": the window of candidate " + std::to_string(f)
                                                   + " does not hold the widest, farthest shifted model plus half an exposure");
               return (int)TLS_OK;
           })))
        return rc;
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)n, words = tlsdev::kTransitWords, units = (size_t)(n_b * n_t * n_s);
    const size_t rows = (size_t)n_k, row_words = (size_t)M + 1;
    // a slab: at most 512 candidates on at most 512 curves, 256 MB of curves (32 bytes a point); the workgroups of a launch:
    // at most 512, 256 MB of scratch (24 bytes a point and 16 bytes a unit each)
    const size_t budget = 256u << 20, stretch = 3 * nn + 2 * units;
    const size_t cs = std::max<size_t>(1, std::min<size_t>({(size_t)n_curves, (size_t)tlsdev::kTransitSlab, budget / (32 * nn)}));
    const size_t sl = std::min<size_t>((size_t)n_fits, (size_t)tlsdev::kTransitSlab);
    const size_t groups = std::max<size_t>(1, std::min<size_t>(sl, budget / (8 * stretch)));
    double2* d_pairs;
    double *d_y, *d_dy, *d_out, *d_period, *d_T0, *d_duration, *d_t, *d_k, *d_profile, *d_impact, *d_ratio, *d_shift, *d_sub, *d_scratch;
    int* d_ints;
    Arena L;
    L.add(d_pairs, cs * nn);            // of one slab, down to the int columns
    L.add(d_y, cs * nn);  L.add(d_dy, cs * nn);  L.add(d_out, sl * words);  L.add(d_period, sl);  L.add(d_T0, sl);
    L.add(d_duration, sl);  L.add(d_ints, 2 * sl);   // slot | row_first
    L.add(d_t, nn);                     // what every slab shares, from here on
    L.add(d_k, rows);  L.add(d_profile, rows * row_words);  L.add(d_impact, (size_t)n_b);  L.add(d_ratio, (size_t)n_t);
    L.add(d_shift, (size_t)n_s);  L.add(d_sub, (size_t)n_sub);  L.add(d_scratch, groups * stretch);
    TLS_HIP(ctx, L.bind(ctx->d_transit));
    if ((rc = ensure_check_counters(ctx))) return rc;
    tlsdev::TimesPairsArgs p;
    p.y = d_y; p.dy = d_dy; p.pairs = d_pairs;
    tlsdev::TransitFitArgs a;
    a.t = d_t; a.pairs = d_pairs; a.slot = d_ints; a.row_first = d_ints + sl; a.period = d_period; a.T0 = d_T0; a.duration = d_duration;
    a.k_rows = d_k; a.profile = d_profile; a.impact = d_impact; a.ratio = d_ratio; a.shift = d_shift; a.sub = d_sub;
    a.scratch = d_scratch; a.out = d_out; a.check = ctx->d_check.ptr; a.window = window; a.delta = delta;
    a.n = (int)n; a.nK = (int)n_k; a.M = (int)M; a.nB = (int)n_b; a.nT = (int)n_t; a.nS = (int)n_s; a.S = (int)n_sub;
    a.min_count = (int)std::min<int64_t>(min_count, INT32_MAX);
    const size_t lds = row_words * 8;
    TLS_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(tlsdev::tls_transit_fit_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    TLS_HIP(ctx, hipMemcpyAsync(d_t, t, nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_k, k_rows, rows * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_profile, profile, rows * row_words * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_impact, impact, (size_t)n_b * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_ratio, ratio, (size_t)n_t * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_shift, shift, (size_t)n_s * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_sub, sub, (size_t)n_sub * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    const SlabStage stage{"transit fit", "tls_transit_fit", curve, n_fits, nn, cs, sl,
                          {{d_y, y}, {d_dy, dy}}, {{d_period, period}, {d_T0, T0}, {d_duration, duration}}, d_ints, 2};
    return run_candidate_slabs(ctx, stage,
        [&](int64_t f, int* at) { at[sl] = (int)row_first[f]; return (size_t)0; },
        [&](const SlabView& s) {
            a.fits = (int)s.fits;
            if (launch_times_pairs(ctx, p, s.curves, nn))
                hipLaunchKernelGGL(tlsdev::tls_transit_fit_kernel, dim3((unsigned)std::min(s.fits, groups)), dim3(tlsdev::kShapeThreads), lds, main_stream(ctx), a);
        },
        [&](const SlabView& s) {
            TLS_HIP(ctx, hipMemcpyAsync(out_records + s.f0, d_out, s.fits * words * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
            return TLS_OK;
        });
}

// ---- the centroid-shift test (tls_centroid.hip.h, DESIGN.md "Centroid test"): the flux and the two centroid rows of the
// curves a slab of candidates reads, then one workgroup a candidate, slab by slab
static_assert(sizeof(tls_centroid_record) == tlsdev::kCentroidWords * 8, "tls_centroid_record is the kernel's record");
static_assert(TLS_CENTROID_MAX_EPOCHS == tlsdev::kCentroidMaxEpochs && TLS_CENTROID_MAX_SHAPE == tlsdev::kCentroidMaxShape,
              "the header's limits");

int tls_centroid_test(tls_ctx* ctx, const double* t, const double* y, const double* cx, const double* cy, int64_t n,
                      int64_t n_curves, const double* period, const double* T0, const double* duration, const int64_t* curve,
                      int64_t n_fits, const double* shape, int64_t L, double window, int64_t min_in, int64_t min_out,
                      int64_t max_epochs, tls_centroid_record* out) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (n_fits < 0 || n_curves < 0 || n < 0) return fail(ctx, TLS_E_ARG, "centroid test: negative count");
    if (!(std::isfinite(window) && window >= 1.0)) return fail(ctx, TLS_E_ARG, "centroid test: the window must be finite and >= 1");
    if (min_in < 1 || min_out < 1) return fail(ctx, TLS_E_ARG, "centroid test: min_in and min_out must be >= 1");
    if (max_epochs < 1 || max_epochs > TLS_CENTROID_MAX_EPOCHS)
        return fail(ctx, TLS_E_ARG, "centroid test: max_epochs out of range [1, 65536]");
    if (L < 2 || L > TLS_CENTROID_MAX_SHAPE) return fail(ctx, TLS_E_ARG, "centroid test: L out of range [2, 2^20]");
    if (!shape) return fail(ctx, TLS_E_ARG, "null argument");
    for (int64_t j = 0; j < L; ++j)
        if (!std::isfinite(shape[j])) return fail(ctx, TLS_E_ARG, "centroid test: the shape must be finite");
    if (n_fits == 0) return TLS_OK;
    if (!t || !y || !cx || !cy || !curve || !period || !T0 || !duration || !out) return fail(ctx, TLS_E_ARG, "null argument");
    int rc;
    if ((rc = check_batch(ctx, "centroid test", n, tlsdev::kCentroidMaxPoints, "[1, 2^22]", n_fits, n_curves))
        || (rc = check_time_stamps(ctx, "centroid test", t, n)) || (rc = check_curves(ctx, "centroid test", curve, n_fits, n_curves)))
        return rc;
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)n, words = tlsdev::kCentroidWords, ll = (size_t)L;
    // a slab: at most 1024 candidates on at most 1024 curves, 256 MB of curves (24 bytes a point); the workgroups of a launch:
    // at most 1024, 256 MB of epoch scratch (72 bytes an epoch beyond those the LDS holds)
    const size_t budget = 256u << 20;
    const size_t cs = std::max<size_t>(1, std::min<size_t>({(size_t)n_curves, 1024, budget / (24 * nn)}));
    const size_t sl = std::min<size_t>((size_t)n_fits, 1024);
    const size_t stretch = max_epochs > tlsdev::kCentroidLdsEpochs
        ? (size_t)(max_epochs - tlsdev::kCentroidLdsEpochs) * tlsdev::kCentroidEpochWords : 0;
    const size_t groups = std::max<size_t>(1, std::min<size_t>({sl, (size_t)tlsdev::kCentroidMaxGroups, stretch ? budget / (8 * stretch) : sl}));
    double *d_y, *d_cx, *d_cy, *d_out, *d_period, *d_T0, *d_duration, *d_t, *d_b, *d_scratch;
    int* d_slot;
    Arena A;
    A.add(d_y, cs * nn);                // of one slab, down to the slots
    A.add(d_cx, cs * nn);  A.add(d_cy, cs * nn);  A.add(d_out, sl * words);  A.add(d_period, sl);  A.add(d_T0, sl);
    A.add(d_duration, sl);  A.add(d_slot, sl);
    A.add(d_t, nn);                     // what every slab shares, from here on
    A.add(d_b, ll);                     // the shape
    A.add(d_scratch, groups * stretch);
    TLS_HIP(ctx, A.bind(ctx->d_centroid));
    if ((rc = ensure_check_counters(ctx))) return rc;
    tlsdev::CentroidArgs a;
    a.t = d_t; a.y = d_y; a.cx = d_cx; a.cy = d_cy; a.slot = d_slot; a.period = d_period; a.T0 = d_T0; a.duration = d_duration;
    a.shape = d_b; a.scratch = d_scratch; a.out = d_out; a.check = ctx->d_check.ptr; a.window = window;
    a.n = (int)n; a.L = (int)L; a.max_epochs = (int)max_epochs;
    a.min_in = (int)std::min<int64_t>(min_in, INT32_MAX);
    a.min_out = (int)std::min<int64_t>(min_out, INT32_MAX);
    TLS_HIP(ctx, hipMemcpyAsync(d_t, t, nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_b, shape, ll * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    const SlabStage stage{"centroid test", "tls_centroid_test", curve, n_fits, nn, cs, sl,
                          {{d_y, y}, {d_cx, cx}, {d_cy, cy}}, {{d_period, period}, {d_T0, T0}, {d_duration, duration}}, d_slot, 1};
    return run_candidate_slabs(ctx, stage, no_int_columns,
        [&](const SlabView& s) {
            a.fits = (int)s.fits;
            hipLaunchKernelGGL(tlsdev::tls_centroid_kernel, dim3((unsigned)std::min(s.fits, groups)), dim3(tlsdev::kCentroidThreads), 0, main_stream(ctx), a);
        },
        [&](const SlabView& s) {
            TLS_HIP(ctx, hipMemcpyAsync(out + s.f0, d_out, s.fits * words * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
            return TLS_OK;
        });
}

// ---- the folded views (tls_views.hip.h, DESIGN.md "Folded views"): one workgroup a candidate, slab by slab; the device writes
// every entry of every output, so the host neither fills nor scatters
static_assert(sizeof(tls_views_record) == tlsdev::kViewsWords * 8, "tls_views_record is the kernel's record");
static_assert(TLS_VIEWS_MAX_BINS == tlsdev::kViewsMaxBins, "the header's limit");

int tls_folded_views(tls_ctx* ctx, const double* t, const double* y, int64_t n, int64_t n_curves, const double* period,
                     const double* T0, const double* duration, const double* secondary_phase, const int64_t* curve,
                     int64_t n_fits, int64_t n_global, int64_t n_local, double local_durations, double local_width,
                     tls_views_record* out, double* global_median, int32_t* global_count, double* local_median,
                     int32_t* local_count) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (n_fits < 0 || n_curves < 0 || n < 0) return fail(ctx, TLS_E_ARG, "folded views: negative count");
    if (n_global < 2 || n_local < 2 || n_global > TLS_VIEWS_MAX_BINS || n_local > TLS_VIEWS_MAX_BINS)
        return fail(ctx, TLS_E_ARG, "folded views: n_global and n_local must lie in [2, 65536]");
    if (!(std::isfinite(local_durations) && local_durations > 0.0))
        return fail(ctx, TLS_E_ARG, "folded views: local_durations must be finite and > 0");
    if (!(std::isfinite(local_width) && local_width > 0.0 && local_width <= 2.0 * local_durations))
        return fail(ctx, TLS_E_ARG, "folded views: local_width must be finite, > 0 and at most 2 * local_durations");
    if (n_fits == 0) return TLS_OK;
    if (!t || !y || !period || !T0 || !duration || !out || !global_median || !global_count || !local_median || !local_count)
        return fail(ctx, TLS_E_ARG, "null argument");
    int rc;
    if ((rc = check_batch(ctx, "folded views", n, tlsdev::kViewsMaxPoints, "[1, 2^20]", n_fits, n_curves))
        || (rc = check_time_stamps(ctx, "folded views", t, n)) || (rc = check_curves(ctx, "folded views", curve, n_fits, n_curves)))
        return rc;
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)n, words = tlsdev::kViewsWords, ng = (size_t)n_global, nl = (size_t)tlsdev::kViewsLocal * (size_t)n_local;
    // a slab: at most 1024 candidates (256 MB of medians and counts, 12 bytes a bin) on at most 1024 curves, 256 MB of curves;
    // the workgroups of a launch: at most 1024, and 256 MB of scratch where the series is longer than the LDS holds
    const size_t budget = 256u << 20;
    const size_t cs = std::max<size_t>(1, std::min<size_t>({(size_t)n_curves, 1024, budget / (8 * nn)}));
    const size_t sl = std::min<size_t>({(size_t)n_fits, (size_t)tlsdev::kViewsSlab, std::max<size_t>(1, budget / (12 * (ng + nl)))});
    const size_t stretch = n > tlsdev::kViewsLdsPoints ? tlsdev::views_scratch_words(nn) : 0;
    const size_t groups = std::max<size_t>(1, std::min<size_t>({sl, (size_t)tlsdev::kViewsMaxGroups, stretch ? budget / (8 * stretch) : sl}));
    double *d_y, *d_out, *d_period, *d_T0, *d_duration, *d_secondary, *d_gmed, *d_lmed, *d_t, *d_scratch;
    int *d_slot, *d_gcnt, *d_lcnt;
    Arena L;
    L.add(d_y, cs * nn);                // of one slab, down to the counts
    L.add(d_out, sl * words);  L.add(d_period, sl);  L.add(d_T0, sl);  L.add(d_duration, sl);
    L.add(d_secondary, sl);             // (held whether or not the call gives secondary phases: the slab's size does not depend on it)
    L.add(d_gmed, sl * ng);  L.add(d_lmed, sl * nl);  L.add(d_slot, sl);  L.add(d_gcnt, sl * ng);  L.add(d_lcnt, sl * nl);
    L.add(d_t, nn);                     // what every slab shares, from here on
    L.add(d_scratch, groups * stretch);
    TLS_HIP(ctx, L.bind(ctx->d_views));
    if ((rc = ensure_check_counters(ctx))) return rc;
    tlsdev::ViewsArgs a;
    a.t = d_t; a.y = d_y; a.slot = d_slot; a.period = d_period; a.T0 = d_T0; a.duration = d_duration;
    a.secondary = secondary_phase ? d_secondary : nullptr;
    a.scratch = d_scratch; a.out = d_out; a.global_median = d_gmed; a.global_count = d_gcnt; a.local_median = d_lmed;
    a.local_count = d_lcnt; a.check = ctx->d_check.ptr; a.k = local_durations; a.width = local_width;
    a.n = (int)n; a.n_global = (int)n_global; a.n_local = (int)n_local;
    TLS_HIP(ctx, hipMemcpyAsync(d_t, t, nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    const SlabStage stage{"folded views", "tls_folded_views", curve, n_fits, nn, cs, sl, {{d_y, y}},
                          {{d_period, period}, {d_T0, T0}, {d_duration, duration}, {d_secondary, secondary_phase}}, d_slot, 1};
    return run_candidate_slabs(ctx, stage, no_int_columns,
        [&](const SlabView& s) {
            a.fits = (int)s.fits;
            hipLaunchKernelGGL(tlsdev::tls_folded_views_kernel, dim3((unsigned)std::min(s.fits, groups)), dim3(tlsdev::kViewsThreads), 0, main_stream(ctx), a);
        },
        [&](const SlabView& s) {
            const size_t f0 = (size_t)s.f0;
            TLS_HIP(ctx, hipMemcpyAsync(out + f0, d_out, s.fits * words * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
            TLS_HIP(ctx, hipMemcpyAsync(global_median + f0 * ng, d_gmed, s.fits * ng * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
            TLS_HIP(ctx, hipMemcpyAsync(global_count + f0 * ng, d_gcnt, s.fits * ng * 4, hipMemcpyDeviceToHost, main_stream(ctx)));
            TLS_HIP(ctx, hipMemcpyAsync(local_median + f0 * nl, d_lmed, s.fits * nl * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
            TLS_HIP(ctx, hipMemcpyAsync(local_count + f0 * nl, d_lcnt, s.fits * nl * 4, hipMemcpyDeviceToHost, main_stream(ctx)));
            return TLS_OK;
        });
}

// ---- the variability periodogram (tls_gls.hip.h, DESIGN.md "Variability periodogram"): the non-uniform DFT of a row matrix,
// the generalised Lomb-Scargle periodogram built on it, and the sine test of a candidate
static_assert(sizeof(tls_sine_record) == tlsdev::kSineWords * 8 && sizeof(tls_sine_harmonic) == tlsdev::kSineHarmonicWords * 8,
              "the sine test's records are the kernel's");
static_assert(TLS_SINE_MAX_HARMONICS == tlsdev::kSineMaxHarmonics && TLS_GLS_MAX_POINTS == tlsdev::kGlsMaxPoints, "the header's limits");

namespace {

int check_gls_axes(tls_ctx* ctx, const double* t, int64_t n, int64_t n_min, const double* f, int64_t F) {
    if (n < n_min || n > TLS_GLS_MAX_POINTS) return fail(ctx, TLS_E_ARG, "periodogram: n out of range");
    if (F < 1 || F > TLS_GLS_MAX_FREQUENCIES) return fail(ctx, TLS_E_ARG, "periodogram: n_freq out of range [1, 2^24]");
    if (!t || !f) return fail(ctx, TLS_E_ARG, "null argument");
    if (int rc = check_time_stamps(ctx, "periodogram", t, n)) return rc;
    for (int64_t k = 0; k < F; ++k)
        if (!(std::isfinite(f[k]) && f[k] > 0.0)) return fail(ctx, TLS_E_ARG, "periodogram: every frequency must be finite and > 0");
    return TLS_OK;
}

// out[r][k] = the (cos, sin) sums of the rows d_A [R][lda] at the frequencies d_f [F], nothing waited for
int enqueue_nudft(tls_ctx* ctx, const double* d_A, int64_t R, int64_t lda, int64_t n, const double* d_t, const double* d_f,
                  int64_t F, double2* d_out) {
    tlsdev::NudftArgs a;
    a.A = d_A; a.t = d_t; a.f = d_f; a.out = d_out; a.lda = (long long)lda; a.R = (int)R; a.n = (int)n; a.F = (int)F;
    const unsigned gx = (unsigned)((F + tlsdev::kGlsFreqTile - 1) / tlsdev::kGlsFreqTile);
    if (R <= tlsdev::kGlsSmallRows)
        hipLaunchKernelGGL(tlsdev::tls_nudft_kernel<1>, dim3(gx, 1), dim3(tlsdev::kGlsThreads), 0, main_stream(ctx), a);
    else
        hipLaunchKernelGGL(tlsdev::tls_nudft_kernel<4>, dim3(gx, (unsigned)((R + tlsdev::kGlsRowTile - 1) / tlsdev::kGlsRowTile)),
                           dim3(tlsdev::kGlsThreads), 0, main_stream(ctx), a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ctx, TLS_E_HIP, std::string("nudft launch: ") + hipGetErrorString(e));
    ctx->last_kernel = "tls_nudft";
    return TLS_OK;
}

// rows of a slab: the sums and spectra of a slab stay below 1 GB, a launch's grid.y below 2^16 tiles of 32 rows
int64_t gls_slab(int64_t rows, int64_t n, int64_t F) {
    const int64_t per_row = 8 * (3 * n + 9 * F) + 1;
    return std::max<int64_t>(1, std::min<int64_t>({rows, (int64_t)32768, (int64_t)(1ll << 30) / per_row}));
}

}  // namespace

int tls_nudft(tls_ctx* ctx, const double* rows, int64_t n_rows, int64_t n, const double* t, const double* frequencies,
              int64_t n_freq, double* out) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (n_rows < 0) return fail(ctx, TLS_E_ARG, "nudft: n_rows < 0");
    int rc = check_gls_axes(ctx, t, n, 1, frequencies, n_freq);
    if (rc || n_rows == 0) return rc;
    if (!rows || !out) return fail(ctx, TLS_E_ARG, "null argument");
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)n, nf = (size_t)n_freq;
    const int64_t slab = gls_slab(n_rows, n, n_freq);
    double2* d_out;
    double *d_rows, *d_t, *d_f;
    Arena L;
    L.add(d_out, (size_t)slab * nf);    // the sums of one slab
    L.add(d_rows, (size_t)slab * nn);   // ... and its rows
    L.add(d_t, nn);  L.add(d_f, nf);
    TLS_HIP(ctx, L.bind(ctx->d_gls));
    TLS_HIP(ctx, hipMemcpyAsync(d_t, t, nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_f, frequencies, nf * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    for (int64_t k0 = 0; k0 < n_rows; k0 += slab) {
        const int64_t R = std::min<int64_t>(slab, n_rows - k0);
        TLS_HIP(ctx, hipMemcpyAsync(d_rows, rows + (size_t)k0 * nn, (size_t)R * nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
        if ((rc = enqueue_nudft(ctx, d_rows, R, n, n, d_t, d_f, n_freq, d_out))) { (void)hipStreamSynchronize(main_stream(ctx)); return rc; }
        TLS_HIP(ctx, hipMemcpyAsync(out + 2 * (size_t)k0 * nf, d_out, (size_t)R * nf * 16, hipMemcpyDeviceToHost, main_stream(ctx)));
        TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));       // (the next slab overwrites the device buffers)
    }
    return TLS_OK;
}

int tls_lomb_scargle(tls_ctx* ctx, const double* t, const double* y, const double* dy, int64_t n, int64_t n_curves,
                     const double* frequencies, int64_t n_freq, double* out_mean, double* out_variance, double* out_power,
                     double* out_amplitude, double* out_phase, int64_t k, double min_separation, tls_peak* out_peaks,
                     int64_t* out_n_peaks, double* out_rows, double* out_weights, double* out_sums) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (n_curves < 0) return fail(ctx, TLS_E_ARG, "periodogram: n_curves < 0");
    int rc = check_gls_axes(ctx, t, n, 3, frequencies, n_freq);
    if (rc) return rc;
    const double ratios[2] = {0.5, 2.0};
    PeaksRequest pk;
    if (k != 0) {
        pk.k = k; pk.sep = min_separation; pk.ratios = ratios; pk.n_ratios = 2; pk.min_power = -INFINITY;
        pk.out = out_peaks; pk.out_n = out_n_peaks;
        if ((rc = check_peaks_request(ctx, pk, n_freq))) return rc;
        if (!out_peaks || !out_n_peaks) return fail(ctx, TLS_E_ARG, "null argument");
    }
    if (n_curves == 0) return TLS_OK;
    if (!y || !out_mean || !out_variance) return fail(ctx, TLS_E_ARG, "null argument");
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)n, nf = (size_t)n_freq;
    const int64_t slab = gls_slab(n_curves, n, n_freq);
    const size_t sl = (size_t)slab, wl = dy ? sl : 1, words = k ? pk.words() : 0;
    double2 *d_yc, *d_cs, *d_cs2;
    double *d_power, *d_amplitude, *d_phase, *d_y, *d_dy, *d_a, *d_w, *d_mean, *d_var, *d_t, *d_f, *d_f2, *d_periods, *d_peaks;
    Arena L;
    L.add(d_yc, sl * nf);               // (YC, YS)
    L.add(d_cs, wl * nf);               // (C, S)
    L.add(d_cs2, wl * nf);              // (C2, S2)
    L.add(d_power, sl * nf);  L.add(d_amplitude, sl * nf);  L.add(d_phase, sl * nf);  L.add(d_y, sl * nn);
    L.add(d_dy, dy ? sl * nn : 0);  L.add(d_a, sl * nn);   // the rows the transform reads
    L.add(d_w, wl * nn);                // ... and their weights
    L.add(d_mean, sl);  L.add(d_var, sl);  L.add(d_t, nn);  L.add(d_f, nf);  L.add(d_f2, nf);   // 2 f
    L.add(d_periods, nf);               // 1 / f
    L.add(d_peaks, sl * words);
    TLS_HIP(ctx, L.bind(ctx->d_gls));
    if (k && (rc = reserve_peak_mask(ctx, slab, n_freq))) return rc;
    std::vector<double> twice(nf), periods(nf), h_peaks(sl * words);
    for (size_t i = 0; i < nf; ++i) { twice[i] = 2.0 * frequencies[i]; periods[i] = 1.0 / frequencies[i]; }
    TLS_HIP(ctx, hipMemcpyAsync(d_t, t, nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_f, frequencies, nf * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_f2, twice.data(), nf * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_periods, periods.data(), nf * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    std::vector<double> h_sums;
    for (int64_t k0 = 0; k0 < n_curves; k0 += slab) {
        const int64_t R = std::min<int64_t>(slab, n_curves - k0), Rw = dy ? R : 1;
        const size_t at = (size_t)k0 * nn, bytes = (size_t)R * nn * 8, spec = (size_t)R * nf * 8;
        TLS_HIP(ctx, hipMemcpyAsync(d_y, y + at, bytes, hipMemcpyHostToDevice, main_stream(ctx)));
        if (dy) TLS_HIP(ctx, hipMemcpyAsync(d_dy, dy + at, bytes, hipMemcpyHostToDevice, main_stream(ctx)));
        tlsdev::GlsPrologueArgs p;
        p.y = d_y; p.dy = d_dy; p.rows = d_a; p.weights = d_w; p.mean = d_mean; p.variance = d_var; p.n = (int)n;
        hipLaunchKernelGGL(tlsdev::tls_gls_prologue_kernel, dim3((unsigned)R), dim3(tlsdev::kGlsThreads), 0, main_stream(ctx), p);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) { (void)hipStreamSynchronize(main_stream(ctx)); return fail(ctx, TLS_E_HIP, std::string("periodogram launch: ") + hipGetErrorString(e)); }
        if ((rc = enqueue_nudft(ctx, d_a, R, n, n, d_t, d_f, n_freq, d_yc))) { (void)hipStreamSynchronize(main_stream(ctx)); return rc; }
        if (dy || k0 == 0) {                         // (the one shared weight row: once)
            if ((rc = enqueue_nudft(ctx, d_w, Rw, n, n, d_t, d_f, n_freq, d_cs))
                || (rc = enqueue_nudft(ctx, d_w, Rw, n, n, d_t, d_f2, n_freq, d_cs2))) { (void)hipStreamSynchronize(main_stream(ctx)); return rc; }
        }
        tlsdev::GlsEpilogueArgs g;
        g.yc = d_yc; g.cs = d_cs; g.cs2 = d_cs2; g.variance = d_var; g.power = d_power; g.amplitude = d_amplitude; g.phase = d_phase;
        g.count = (long long)R * (long long)n_freq; g.F = (int)n_freq; g.shared_weights = dy ? 0 : 1;
        const unsigned blocks = (unsigned)std::min<long long>((g.count + tlsdev::kGlsThreads - 1) / tlsdev::kGlsThreads, 16384);
        hipLaunchKernelGGL(tlsdev::tls_gls_epilogue_kernel, dim3(blocks), dim3(tlsdev::kGlsThreads), 0, main_stream(ctx), g);
        e = hipGetLastError();
        if (e != hipSuccess) { (void)hipStreamSynchronize(main_stream(ctx)); return fail(ctx, TLS_E_HIP, std::string("periodogram launch: ") + hipGetErrorString(e)); }
        if (k && (rc = enqueue_find_peaks(ctx, pk, R, n_freq, d_power, nf, d_periods, nullptr, nullptr, nullptr, nullptr, d_peaks))) {
            (void)hipStreamSynchronize(main_stream(ctx));
            return rc;
        }
        ctx->last_kernel = "tls_lomb_scargle";
        TLS_HIP(ctx, hipMemcpyAsync(out_mean + k0, d_mean, (size_t)R * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        TLS_HIP(ctx, hipMemcpyAsync(out_variance + k0, d_var, (size_t)R * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        if (out_power) TLS_HIP(ctx, hipMemcpyAsync(out_power + (size_t)k0 * nf, d_power, spec, hipMemcpyDeviceToHost, main_stream(ctx)));
        if (out_amplitude) TLS_HIP(ctx, hipMemcpyAsync(out_amplitude + (size_t)k0 * nf, d_amplitude, spec, hipMemcpyDeviceToHost, main_stream(ctx)));
        if (out_phase) TLS_HIP(ctx, hipMemcpyAsync(out_phase + (size_t)k0 * nf, d_phase, spec, hipMemcpyDeviceToHost, main_stream(ctx)));
        if (out_rows) TLS_HIP(ctx, hipMemcpyAsync(out_rows + at, d_a, bytes, hipMemcpyDeviceToHost, main_stream(ctx)));
        if (out_weights && (dy || k0 == 0))
            TLS_HIP(ctx, hipMemcpyAsync(out_weights + (dy ? at : 0), d_w, (size_t)Rw * nn * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        if (k) TLS_HIP(ctx, hipMemcpyAsync(h_peaks.data(), d_peaks, (size_t)R * words * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        if (out_sums) {
            h_sums.resize(2 * ((size_t)R + 2 * (size_t)Rw) * nf);
            TLS_HIP(ctx, hipMemcpyAsync(h_sums.data(), d_yc, (size_t)R * nf * 16, hipMemcpyDeviceToHost, main_stream(ctx)));
            TLS_HIP(ctx, hipMemcpyAsync(h_sums.data() + 2 * (size_t)R * nf, d_cs, (size_t)Rw * nf * 16, hipMemcpyDeviceToHost, main_stream(ctx)));
            TLS_HIP(ctx, hipMemcpyAsync(h_sums.data() + 2 * ((size_t)R + (size_t)Rw) * nf, d_cs2, (size_t)Rw * nf * 16, hipMemcpyDeviceToHost, main_stream(ctx)));
        }
        TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));       // (the next slab overwrites the device buffers)
        if (k) for (int64_t c = 0; c < R; ++c) read_peaks(pk, h_peaks.data(), c, k0 + c);
        if (out_sums) {
            const double* yc = h_sums.data();
            const double* cs = yc + 2 * (size_t)R * nf;
            const double* cs2 = cs + 2 * (size_t)Rw * nf;
            for (size_t r = 0; r < (size_t)R; ++r)
                for (size_t q = 0; q < nf; ++q) {
                    double* o = out_sums + 6 * (((size_t)k0 + r) * nf + q);
                    const size_t w = 2 * ((dy ? r : 0) * nf + q);
                    o[0] = yc[2 * (r * nf + q)]; o[1] = yc[2 * (r * nf + q) + 1];
                    o[2] = cs[w]; o[3] = cs[w + 1]; o[4] = cs2[w]; o[5] = cs2[w + 1];
                }
        }
    }
    return TLS_OK;
}

int tls_sine_test(tls_ctx* ctx, const double* t, const double* y, const double* dy, int64_t n, int64_t n_curves,
                  const double* period, const double* T0, const double* duration, const int64_t* curve, int64_t n_fits,
                  const double* harmonics, int64_t n_harmonics, double mask, tls_sine_record* out, tls_sine_harmonic* out_harmonics,
                  double* out_sums) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (n_fits < 0 || n_curves < 0 || n < 0) return fail(ctx, TLS_E_ARG, "sine test: negative count");
    if (n_harmonics < 1 || n_harmonics > TLS_SINE_MAX_HARMONICS) return fail(ctx, TLS_E_ARG, "sine test: n_harmonics out of range [1, 8]");
    if (!harmonics) return fail(ctx, TLS_E_ARG, "null argument");
    for (int64_t h = 0; h < n_harmonics; ++h)
        if (!(std::isfinite(harmonics[h]) && harmonics[h] > 0.0)) return fail(ctx, TLS_E_ARG, "sine test: every harmonic must be finite and > 0");
    if (!(std::isfinite(mask) && mask >= 0.0)) return fail(ctx, TLS_E_ARG, "sine test: mask must be finite and >= 0");
    if ((T0 == nullptr) != (duration == nullptr)) return fail(ctx, TLS_E_ARG, "sine test: T0 and duration come together");
    if (n_fits == 0) return TLS_OK;
    if (!t || !y || !curve || !period || !out || !out_harmonics) return fail(ctx, TLS_E_ARG, "null argument");
    int rc;
    if ((rc = check_batch(ctx, "sine test", n, TLS_GLS_MAX_POINTS, "[1, 2^22]", n_fits, n_curves))
        || (rc = check_time_stamps(ctx, "sine test", t, n)) || (rc = check_curves(ctx, "sine test", curve, n_fits, n_curves)))
        return rc;
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)n, nH = (size_t)n_harmonics;
    // a slab: at most 1024 candidates on at most 1024 curves, 256 MB of curves
    const size_t cs = std::max<size_t>(1, std::min<size_t>({(size_t)n_curves, 1024, (256u << 20) / (16 * nn)}));
    const size_t sl = std::min<size_t>((size_t)n_fits, 1024);
    double *d_y, *d_dy, *d_out, *d_out_h, *d_sums, *d_period, *d_T0, *d_duration, *d_t, *d_harmonics;
    int* d_slot;
    Arena L;
    L.add(d_y, cs * nn);                // of one slab, down to the slots
    L.add(d_dy, cs * nn);  L.add(d_out, sl * tlsdev::kSineWords);  L.add(d_out_h, sl * nH * tlsdev::kSineHarmonicWords);
    L.add(d_sums, sl * nH * 6);  L.add(d_period, sl);  L.add(d_T0, sl);  L.add(d_duration, sl);  L.add(d_slot, sl);
    L.add(d_t, nn);                     // what every slab shares, from here on
    L.add(d_harmonics, nH);
    TLS_HIP(ctx, L.bind(ctx->d_gls));
    tlsdev::SineArgs a;
    a.t = d_t; a.y = d_y; a.dy = dy ? d_dy : nullptr; a.slot = d_slot; a.period = d_period;
    a.T0 = T0 ? d_T0 : nullptr; a.duration = T0 ? d_duration : nullptr; a.harmonics = d_harmonics;
    a.out = d_out; a.out_h = d_out_h; a.out_sums = out_sums ? d_sums : nullptr; a.mask = mask; a.n = (int)n; a.nH = (int)n_harmonics;
    TLS_HIP(ctx, hipMemcpyAsync(d_t, t, nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_harmonics, harmonics, nH * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    const SlabStage stage{"sine test", "tls_sine_test", curve, n_fits, nn, cs, sl,
                          {{d_y, y}, {d_dy, dy}}, {{d_period, period}, {d_T0, T0}, {d_duration, duration}}, d_slot, 1};
    return run_candidate_slabs(ctx, stage, no_int_columns,
        [&](const SlabView& s) {
            a.fits = (int)s.fits;
            hipLaunchKernelGGL(tlsdev::tls_sine_test_kernel, dim3((unsigned)s.fits), dim3(tlsdev::kSineThreads), 0, main_stream(ctx), a);
        },
        [&](const SlabView& s) {
            const size_t f0 = (size_t)s.f0;
            TLS_HIP(ctx, hipMemcpyAsync(out + f0, d_out, s.fits * sizeof(tls_sine_record), hipMemcpyDeviceToHost, main_stream(ctx)));
            TLS_HIP(ctx, hipMemcpyAsync(out_harmonics + f0 * nH, d_out_h, s.fits * nH * sizeof(tls_sine_harmonic), hipMemcpyDeviceToHost, main_stream(ctx)));
            if (out_sums) TLS_HIP(ctx, hipMemcpyAsync(out_sums + f0 * nH * 6, d_sums, s.fits * nH * 48, hipMemcpyDeviceToHost, main_stream(ctx)));
            return TLS_OK;
        });
}

// ---- pre-whitening (tls_prewhiten.hip.h, DESIGN.md "Pre-whitening"): the periodogram's kernels and the step kernel, iteration
// by iteration on rows that stay on the device; the host reads one count an iteration
static_assert(sizeof(tls_prewhiten_term) == tlsdev::kPrewhitenWords * 8, "tls_prewhiten_term is the kernel's record");
static_assert(TLS_PREWHITEN_MAX_TERMS == tlsdev::kPrewhitenMaxTerms && TLS_PREWHITEN_LDS_POINTS == tlsdev::kPrewhitenLdsPoints,
              "the header's limits");

// tls_prewhiten (masked false: mask is not looked at) and tls_prewhiten_masked, whose weights are the curve's own as with a dy
static int prewhiten(tls_ctx* ctx, const double* t, const double* y, const double* dy, bool masked, const uint8_t* mask, int64_t n,
                     int64_t n_curves, const double* frequencies, int64_t n_freq, int64_t n_terms, int64_t n_harmonics,
                     double min_power, double* out_flat, double* out_trend, tls_prewhiten_term* out_terms,
                     int64_t* out_n_iterations, double* out_status, double* out_steps, double* out_sums) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (n_curves < 0) return fail(ctx, TLS_E_ARG, "prewhiten: n_curves < 0");
    int rc = check_gls_axes(ctx, t, n, 3, frequencies, n_freq);
    if (rc) return rc;
    if (n_terms < 1 || n_terms > TLS_PREWHITEN_MAX_TERMS) return fail(ctx, TLS_E_ARG, "prewhiten: n_terms out of range [1, 32]");
    if (n_harmonics < 1 || n_harmonics > TLS_SINE_MAX_HARMONICS) return fail(ctx, TLS_E_ARG, "prewhiten: n_harmonics out of range [1, 8]");
    if (!(min_power >= 0.0 && min_power <= 1.0)) return fail(ctx, TLS_E_ARG, "prewhiten: min_power must lie in [0, 1]");
    if (n_curves == 0) return TLS_OK;
    if (!y || !out_flat || !out_terms || !out_n_iterations || !out_status || (masked && !mask)) return fail(ctx, TLS_E_ARG, "null argument");
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    const bool own = dy || masked;                   // every curve has a weight row of its own
    const size_t nn = (size_t)n, nf = (size_t)n_freq, K = (size_t)n_terms, KH = K * (size_t)n_harmonics;
    const size_t words = tlsdev::kPrewhitenWords;
    // rows of a slab: the rows, sums and spectra of a slab stay below 1 GB, and at most 4096 curves
    const size_t per_row = 8 * ((out_steps ? 7 + KH : 6) * nn + 9 * nf + KH * (words + 6) + 8);
    const size_t sl = std::max<size_t>(1, std::min<size_t>({(size_t)n_curves, 4096, ((size_t)1 << 30) / per_row}));
    const size_t wl = own ? sl : 1;
    if (masked) TLS_HIP(ctx, ctx->d_protect_bytes.reserve(sl * nn));
    const unsigned char* d_mask = masked ? ctx->d_protect_bytes.ptr : nullptr;
    double2 *d_yc, *d_cs, *d_cs2;
    double *d_power, *d_amplitude, *d_phase, *d_y, *d_r, *d_dy, *d_a, *d_w, *d_trend, *d_mean0, *d_mean, *d_var, *d_status, *d_terms,
        *d_sums, *d_t, *d_f, *d_f2, *d_steps;
    long long* d_iterations;
    unsigned long long* d_counts;
    int* d_active;
    Arena L;
    L.add(d_yc, sl * nf);               // (YC, YS)
    L.add(d_cs, wl * nf);               // (C, S)
    L.add(d_cs2, wl * nf);              // (C2, S2)
    L.add(d_power, sl * nf);  L.add(d_amplitude, sl * nf);  L.add(d_phase, sl * nf);  L.add(d_y, sl * nn);  L.add(d_r, sl * nn);
    L.add(d_dy, dy ? sl * nn : 0);  L.add(d_a, sl * nn);   // (flat at the end)
    L.add(d_w, wl * nn);  L.add(d_trend, sl * nn);  L.add(d_mean0, sl);  L.add(d_mean, sl);  L.add(d_var, sl);
    L.add(d_status, sl);  L.add(d_terms, sl * KH * words);  L.add(d_sums, sl * KH * 6);  L.add(d_t, nn);  L.add(d_f, nf);
    L.add(d_f2, nf);                    // 2 f
    L.add(d_iterations, sl);  L.add(d_counts, K);   // (behind the iterations: one memset clears both)
    L.add(d_active, sl);  L.add(d_steps, out_steps ? (KH + 1) * sl * nn : 0);
    TLS_HIP(ctx, L.bind(ctx->d_gls));
    const bool lds = n <= tlsdev::kPrewhitenLdsPoints;
    const size_t lds_bytes = tlsdev::prewhiten_lds_bytes((int)n, lds);
    auto step_kernel = lds ? tlsdev::tls_prewhiten_step_kernel<true> : tlsdev::tls_prewhiten_step_kernel<false>;
    auto step_masked_kernel = lds ? tlsdev::tls_prewhiten_step_masked_kernel<true> : tlsdev::tls_prewhiten_step_masked_kernel<false>;
    TLS_HIP(ctx, hipFuncSetAttribute(masked ? reinterpret_cast<const void*>(step_masked_kernel) : reinterpret_cast<const void*>(step_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    std::vector<double> twice(nf);
    for (size_t i = 0; i < nf; ++i) twice[i] = 2.0 * frequencies[i];
    // a term that was not reached: status 2, NaN elsewhere
    std::vector<double> blank(sl * KH * (words + 6), (double)NAN);
    for (size_t q = 0; q < sl * KH; ++q) blank[q * words] = 2.0;
    std::vector<int> ones(sl, 1);
    TLS_HIP(ctx, hipMemcpyAsync(d_t, t, nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_f, frequencies, nf * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_f2, twice.data(), nf * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    auto launched = [&](const char* what) -> int {
        const hipError_t e = hipGetLastError();
        if (e == hipSuccess) return TLS_OK;
        (void)hipStreamSynchronize(main_stream(ctx));
        return fail(ctx, TLS_E_HIP, std::string("prewhiten ") + what + " launch: " + hipGetErrorString(e));
    };
    for (int64_t k0 = 0; k0 < n_curves; k0 += (int64_t)sl) {
        const int64_t R = std::min<int64_t>((int64_t)sl, n_curves - k0), Rw = own ? R : 1;
        const size_t at = (size_t)k0 * nn, rows = (size_t)R, bytes = rows * nn * 8;
        TLS_HIP(ctx, hipMemcpyAsync(d_y, y + at, bytes, hipMemcpyHostToDevice, main_stream(ctx)));
        TLS_HIP(ctx, hipMemcpyAsync(d_r, d_y, bytes, hipMemcpyDeviceToDevice, main_stream(ctx)));
        if (dy) TLS_HIP(ctx, hipMemcpyAsync(d_dy, dy + at, bytes, hipMemcpyHostToDevice, main_stream(ctx)));
        if (masked) TLS_HIP(ctx, hipMemcpyAsync(ctx->d_protect_bytes.ptr, mask + at, rows * nn, hipMemcpyHostToDevice, main_stream(ctx)));
        TLS_HIP(ctx, hipMemsetAsync(d_trend, 0, bytes, main_stream(ctx)));
        TLS_HIP(ctx, hipMemsetAsync(d_status, 0, rows * 8, main_stream(ctx)));
        TLS_HIP(ctx, hipMemsetAsync(d_iterations, 0, (sl + K) * 8, main_stream(ctx)));            // (and the counts behind them)
        TLS_HIP(ctx, hipMemcpyAsync(d_active, ones.data(), rows * 4, hipMemcpyHostToDevice, main_stream(ctx)));
        TLS_HIP(ctx, hipMemcpyAsync(d_terms, blank.data(), rows * KH * words * 8, hipMemcpyHostToDevice, main_stream(ctx)));
        TLS_HIP(ctx, hipMemcpyAsync(d_sums, blank.data() + sl * KH * words, rows * KH * 48, hipMemcpyHostToDevice, main_stream(ctx)));
        int64_t ran = 0;
        for (int64_t j = 0; j < n_terms; ++j) {
            tlsdev::GlsPrologueArgs p;
            p.y = d_r; p.dy = d_dy; p.rows = d_a; p.weights = d_w; p.mean = j == 0 ? d_mean0 : d_mean; p.variance = d_var; p.n = (int)n;
            if (masked) hipLaunchKernelGGL(tlsdev::tls_gls_prologue_masked_kernel, dim3((unsigned)R), dim3(tlsdev::kGlsThreads), 0, main_stream(ctx), p, d_mask);
            else hipLaunchKernelGGL(tlsdev::tls_gls_prologue_kernel, dim3((unsigned)R), dim3(tlsdev::kGlsThreads), 0, main_stream(ctx), p);
            if ((rc = launched("prologue"))) return rc;
            if ((rc = enqueue_nudft(ctx, d_a, R, n, n, d_t, d_f, n_freq, d_yc))) { (void)hipStreamSynchronize(main_stream(ctx)); return rc; }
            if (j == 0 && (own || k0 == 0)) {         // (the sums of the weights: once a call, or once a slab with dy)
                if ((rc = enqueue_nudft(ctx, d_w, Rw, n, n, d_t, d_f, n_freq, d_cs))
                    || (rc = enqueue_nudft(ctx, d_w, Rw, n, n, d_t, d_f2, n_freq, d_cs2))) { (void)hipStreamSynchronize(main_stream(ctx)); return rc; }
            }
            tlsdev::GlsEpilogueArgs g;
            g.yc = d_yc; g.cs = d_cs; g.cs2 = d_cs2; g.variance = d_var; g.power = d_power; g.amplitude = d_amplitude; g.phase = d_phase;
            g.count = (long long)R * (long long)n_freq; g.F = (int)n_freq; g.shared_weights = own ? 0 : 1;
            const unsigned blocks = (unsigned)std::min<long long>((g.count + tlsdev::kGlsThreads - 1) / tlsdev::kGlsThreads, 16384);
            hipLaunchKernelGGL(tlsdev::tls_gls_epilogue_kernel, dim3(blocks), dim3(tlsdev::kGlsThreads), 0, main_stream(ctx), g);
            if ((rc = launched("epilogue"))) return rc;
            tlsdev::PrewhitenArgs a;
            a.t = d_t; a.f = d_f; a.dy = d_dy; a.power = d_power; a.r = d_r; a.trend = d_trend; a.terms = d_terms; a.sums = d_sums;
            a.steps = d_steps; a.active = d_active; a.n_iterations = d_iterations; a.status = d_status; a.counts = d_counts;
            a.min_power = min_power; a.n = (int)n; a.F = (int)n_freq; a.R = (int)R; a.K = (int)n_terms; a.H = (int)n_harmonics; a.j = (int)j;
            if (masked) hipLaunchKernelGGL(step_masked_kernel, dim3((unsigned)R), dim3(tlsdev::kPrewhitenThreads), lds_bytes, main_stream(ctx), a, d_mask);
            else hipLaunchKernelGGL(step_kernel, dim3((unsigned)R), dim3(tlsdev::kPrewhitenThreads), lds_bytes, main_stream(ctx), a);
            if ((rc = launched("step"))) return rc;
            ctx->last_kernel = masked ? "tls_prewhiten_masked" : "tls_prewhiten";
            ran = j + 1;
            if (j + 1 < n_terms) {
                unsigned long long going = 0;
                TLS_HIP(ctx, hipMemcpyAsync(&going, d_counts + j, 8, hipMemcpyDeviceToHost, main_stream(ctx)));
                TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));
                if (going == 0) break;
            }
        }
        // (the steps no iteration reached, and the one behind the last, hold the final rows)
        if (d_steps)
            for (size_t s = (size_t)ran * (size_t)n_harmonics; s <= KH; ++s)
                TLS_HIP(ctx, hipMemcpyAsync(d_steps + s * rows * nn, d_r, bytes, hipMemcpyDeviceToDevice, main_stream(ctx)));
        tlsdev::PrewhitenFinishArgs fin;
        fin.y = d_y; fin.mean0 = d_mean0; fin.trend = d_trend; fin.flat = d_a; fin.count = (long long)R * (long long)n; fin.n = (int)n;
        const unsigned fblocks = (unsigned)std::min<long long>((fin.count + tlsdev::kPrewhitenThreads - 1) / tlsdev::kPrewhitenThreads, 16384);
        hipLaunchKernelGGL(tlsdev::tls_prewhiten_finish_kernel, dim3(fblocks), dim3(tlsdev::kPrewhitenThreads), 0, main_stream(ctx), fin);
        if ((rc = launched("finish"))) return rc;
        TLS_HIP(ctx, hipMemcpyAsync(out_flat + at, d_a, bytes, hipMemcpyDeviceToHost, main_stream(ctx)));
        if (out_trend) TLS_HIP(ctx, hipMemcpyAsync(out_trend + at, d_trend, bytes, hipMemcpyDeviceToHost, main_stream(ctx)));
        TLS_HIP(ctx, hipMemcpyAsync(out_terms + (size_t)k0 * KH, d_terms, rows * KH * words * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        TLS_HIP(ctx, hipMemcpyAsync(out_n_iterations + k0, d_iterations, rows * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        TLS_HIP(ctx, hipMemcpyAsync(out_status + k0, d_status, rows * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        if (out_sums) TLS_HIP(ctx, hipMemcpyAsync(out_sums + (size_t)k0 * KH * 6, d_sums, rows * KH * 48, hipMemcpyDeviceToHost, main_stream(ctx)));
        if (out_steps)
            for (size_t s = 0; s <= KH; ++s)
                TLS_HIP(ctx, hipMemcpyAsync(out_steps + s * (size_t)n_curves * nn + at, d_steps + s * rows * nn, bytes,
                                            hipMemcpyDeviceToHost, main_stream(ctx)));
        TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));       // (the next slab overwrites the device buffers)
    }
    return TLS_OK;
}

int tls_prewhiten(tls_ctx* ctx, const double* t, const double* y, const double* dy, int64_t n, int64_t n_curves,
                  const double* frequencies, int64_t n_freq, int64_t n_terms, int64_t n_harmonics, double min_power,
                  double* out_flat, double* out_trend, tls_prewhiten_term* out_terms, int64_t* out_n_iterations,
                  double* out_status, double* out_steps, double* out_sums) {
    return prewhiten(ctx, t, y, dy, false, nullptr, n, n_curves, frequencies, n_freq, n_terms, n_harmonics, min_power, out_flat,
                     out_trend, out_terms, out_n_iterations, out_status, out_steps, out_sums);
}

int tls_prewhiten_masked(tls_ctx* ctx, const double* t, const double* y, const double* dy, const uint8_t* mask, int64_t n,
                         int64_t n_curves, const double* frequencies, int64_t n_freq, int64_t n_terms, int64_t n_harmonics,
                         double min_power, double* out_flat, double* out_trend, tls_prewhiten_term* out_terms,
                         int64_t* out_n_iterations, double* out_status, double* out_steps, double* out_sums) {
    return prewhiten(ctx, t, y, dy, true, mask, n, n_curves, frequencies, n_freq, n_terms, n_harmonics, min_power, out_flat,
                     out_trend, out_terms, out_n_iterations, out_status, out_steps, out_sums);
}

// ---- the ephemeris match (tls_match.hip.h, DESIGN.md "Ephemeris match"): every candidate against every other, the g range in
// chunks along gridDim.y, then the chunks' partial records combined
static_assert(sizeof(tls_match_record) == tlsdev::kMatchWords * 8, "tls_match_record is the kernel's record");
static_assert(TLS_MATCH_MAX_CANDIDATES == tlsdev::kMatchMaxCandidates && TLS_MATCH_MAX_RATIO == tlsdev::kMatchMaxRatio, "the header's limits");
static_assert(sizeof(tlsdev::MatchPartial) % 8 == 0, "partial records lie in a buffer of doubles");

int tls_ephemeris_match(tls_ctx* ctx, const int64_t* star, const double* period, const double* T0, const double* duration,
                        const double* strength, int64_t n, double span, double drift_tolerance, double epoch_tolerance,
                        int64_t max_ratio, tls_match_record* out) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (!(std::isfinite(span) && span > 0.0)) return fail(ctx, TLS_E_ARG, "ephemeris match: span must be finite and > 0");
    if (!(std::isfinite(drift_tolerance) && drift_tolerance >= 0.0))
        return fail(ctx, TLS_E_ARG, "ephemeris match: drift_tolerance must be finite and >= 0");
    if (!(std::isfinite(epoch_tolerance) && epoch_tolerance >= 0.0))
        return fail(ctx, TLS_E_ARG, "ephemeris match: epoch_tolerance must be finite and >= 0");
    if (max_ratio < 1 || max_ratio > TLS_MATCH_MAX_RATIO) return fail(ctx, TLS_E_ARG, "ephemeris match: max_ratio out of range [1, 64]");
    if (n < 0 || n > TLS_MATCH_MAX_CANDIDATES) return fail(ctx, TLS_E_ARG, "ephemeris match: n out of range [0, 2^20]");
    if (n == 0) return TLS_OK;
    if (!star || !period || !T0 || !duration || !strength || !out) return fail(ctx, TLS_E_ARG, "null argument");
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)n, words = (size_t)tlsdev::kMatchWords;
    const int tiles = (int)((n + tlsdev::kMatchTile - 1) / tlsdev::kMatchTile);
    const int chunks = tlsdev::match_chunks(tiles);
    long long* d_star;
    double *d_period, *d_T0, *d_duration, *d_strength, *d_out;
    tlsdev::MatchPartial* d_partial;
    Arena L;
    L.add(d_star, nn);  L.add(d_period, nn);  L.add(d_T0, nn);  L.add(d_duration, nn);  L.add(d_strength, nn);
    L.add(d_out, words * nn);                 // records
    L.add(d_partial, (size_t)chunks * nn);    // ... and the partial records of every chunk
    TLS_HIP(ctx, L.bind(ctx->d_match));
    TLS_HIP(ctx, hipMemcpyAsync(d_star, star, nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_period, period, nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_T0, T0, nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_duration, duration, nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_strength, strength, nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    tlsdev::MatchArgs a;
    a.star = d_star;
    a.period = d_period; a.T0 = d_T0; a.duration = d_duration; a.strength = d_strength;
    a.partial = d_partial; a.out = d_out;
    a.span = span; a.drift_tolerance = drift_tolerance; a.epoch_tolerance = epoch_tolerance; a.max_ratio = (double)max_ratio;
    a.n = (int)n; a.tiles = tiles; a.chunks = chunks;
    hipLaunchKernelGGL(tlsdev::tls_match_pairs_kernel, dim3((unsigned)tiles, (unsigned)chunks), dim3(tlsdev::kMatchTile), 0,
                       main_stream(ctx), a);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        hipLaunchKernelGGL(tlsdev::tls_match_combine_kernel, dim3((unsigned)tiles), dim3(tlsdev::kMatchTile), 0, main_stream(ctx), a);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(main_stream(ctx));
        return fail(ctx, TLS_E_HIP, std::string("ephemeris match launch: ") + hipGetErrorString(e));
    }
    ctx->last_kernel = "tls_ephemeris_match";
    TLS_HIP(ctx, hipMemcpyAsync(out, d_out, words * nn * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
    TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));
    return TLS_OK;
}

// ---- the noise profile (tls_noise.hip.h, DESIGN.md "Noise profile"): a curve kernel (median, sigma, the clipped points, the
// point-to-point sigma), then one workgroup a (width, curve)
static_assert(sizeof(tls_noise_curve) == tlsdev::kNoiseWords * 8, "tls_noise_curve is the kernel's record");
static_assert(TLS_NOISE_MAX_WIDTH == tlsdev::kNoiseMaxWidth && TLS_NOISE_MAX_WIDTHS == tlsdev::kNoiseMaxWidths &&
              TLS_NOISE_LDS_POINTS == tlsdev::kNoiseLdsPoints, "the header's limits");
static_assert(tlsdev::noise_width_lds_bytes(tlsdev::kNoiseLdsPoints, true) <= 160 * 1024, "the longest resident row fits the LDS");

int tls_noise_profile(tls_ctx* ctx, const double* t, const double* y, int64_t n, int64_t n_curves, const int64_t* widths,
                      const double* span_max, int64_t n_widths, double pair_span, double clip_upper, double clip_lower,
                      int64_t min_count, tls_noise_curve* out_curves, int64_t* out_count, double* out_robust, double* out_rms) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (n < 3 || n > TLS_NOISE_MAX_POINTS) return fail(ctx, TLS_E_ARG, "noise profile: n out of range [3, 2^22]");
    if (n_curves < 0) return fail(ctx, TLS_E_ARG, "noise profile: n_curves < 0");
    if (n_widths < 1 || n_widths > TLS_NOISE_MAX_WIDTHS) return fail(ctx, TLS_E_ARG, "noise profile: n_widths out of range [1, 64]");
    if (!widths || !span_max) return fail(ctx, TLS_E_ARG, "null argument");
    for (int64_t k = 0; k < n_widths; ++k) {
        if (widths[k] < 1 || widths[k] > n || widths[k] > TLS_NOISE_MAX_WIDTH || (k > 0 && widths[k] <= widths[k - 1]))
            return fail(ctx, TLS_E_ARG, "noise profile: the widths must ascend strictly within [1, min(n, " + std::to_string(TLS_NOISE_MAX_WIDTH) + ")]");
        if (!(span_max[k] >= 0.0)) return fail(ctx, TLS_E_ARG, "noise profile: every span_max must be >= 0");
    }
    if (!(pair_span >= 0.0)) return fail(ctx, TLS_E_ARG, "noise profile: pair_span must be >= 0");
    if (!(clip_upper >= 0.0) || !(clip_lower >= 0.0)) return fail(ctx, TLS_E_ARG, "noise profile: the clips must be >= 0");
    if (min_count < 1) return fail(ctx, TLS_E_ARG, "noise profile: min_count < 1");
    if (n_curves == 0) return TLS_OK;
    if (!y || !out_curves || !out_count || !out_robust || !out_rms) return fail(ctx, TLS_E_ARG, "null argument");
    const size_t nn = (size_t)n, W = (size_t)n_widths;
    if ((uint64_t)n_curves > (uint64_t)(SIZE_MAX / 8) / (uint64_t)n) return fail(ctx, TLS_E_ARG, "noise profile: rows too large");
    if (t)
        for (size_t i = 0; i < nn; ++i)
            if (!std::isfinite(t[i]) || (i > 0 && t[i] < t[i - 1])) return fail(ctx, TLS_E_ARG, "noise profile: t must be finite and ascending");
    for (size_t q = 0; q < (size_t)n_curves * nn; ++q)
        if (!std::isfinite(y[q])) return fail(ctx, TLS_E_ARG, "noise profile: row " + std::to_string(q / nn) + " has a non-finite value");
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    const bool lds = n <= tlsdev::kNoiseLdsPoints;
    const size_t mask_words = tlsdev::noise_mask_words((int)n);
    // curves per launch: at most 256 MB of rows, at most 256 MB of window means where they lie in device memory, and
    // gridDim.y within its limit
    int64_t slab = std::min<int64_t>({n_curves, (int64_t)65535, (int64_t)((256u << 20) / (8 * nn))});
    if (!lds) slab = std::min<int64_t>(slab, (int64_t)((256u << 20) / (8 * nn * W)));
    slab = std::max<int64_t>(1, slab);
    const size_t S = (size_t)slab;
    double *d_t, *d_span, *d_y, *d_d, *d_records, *d_robust, *d_rms, *d_v;
    int* d_widths;
    long long* d_count;
    unsigned int* d_bad;
    unsigned long long* d_mask;
    Arena L;
    L.add(d_t, nn);  L.add(d_span, W);  L.add(d_widths, W);
    L.add(d_y, S * nn);                       // of one slab, from here on
    L.add(d_d, S * nn);  L.add(d_records, S * tlsdev::kNoiseWords);  L.add(d_count, S * W);  L.add(d_robust, S * W);
    L.add(d_rms, S * W);  L.add(d_bad, S * (nn + 1));   // clip counts
    // for rows that do not fit the LDS: the window means and validity words of every (curve, width)
    L.add(d_v, lds ? 0 : S * W * nn);  L.add(d_mask, lds ? 0 : S * W * mask_words);
    TLS_HIP(ctx, L.bind(ctx->d_noise));
    std::vector<int> w32((size_t)n_widths);
    for (size_t k = 0; k < W; ++k) w32[k] = (int)widths[k];
    if (t) TLS_HIP(ctx, hipMemcpyAsync(d_t, t, nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_span, span_max, W * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_widths, w32.data(), W * 4, hipMemcpyHostToDevice, main_stream(ctx)));
    const size_t curve_lds = tlsdev::noise_curve_lds_bytes((int)n, lds), width_lds = tlsdev::noise_width_lds_bytes((int)n, lds);
    auto curve_kernel = lds ? tlsdev::tls_noise_curve_kernel<true> : tlsdev::tls_noise_curve_kernel<false>;
    auto width_kernel = lds ? tlsdev::tls_noise_width_kernel<true> : tlsdev::tls_noise_width_kernel<false>;
    TLS_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(curve_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)curve_lds));
    TLS_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(width_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)width_lds));
    tlsdev::NoiseArgs a;
    a.t = t ? d_t : nullptr; a.y = d_y; a.d = d_d; a.bad = d_bad; a.records = d_records;
    a.widths = d_widths; a.span_max = d_span;
    a.v = d_v; a.mask = d_mask;
    a.count = d_count; a.robust = d_robust; a.rms = d_rms; a.check = nullptr;
    a.pair_span = pair_span; a.clip_upper = clip_upper; a.clip_lower = clip_lower;
    a.n = (int)n; a.W = (int)n_widths; a.min_count = (int)std::min<int64_t>(min_count, (int64_t)INT32_MAX);
#ifdef TLS_DEBUG_CHECKS
    if (int rc = ensure_check_counters(ctx)) return rc;
    a.check = ctx->d_check.ptr;
#endif
    for (int64_t k0 = 0; k0 < n_curves; k0 += slab) {
        const size_t rows = (size_t)std::min<int64_t>(slab, n_curves - k0);
        TLS_HIP(ctx, hipMemcpyAsync(d_y, y + (size_t)k0 * nn, rows * nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
        hipLaunchKernelGGL(curve_kernel, dim3((unsigned)rows), dim3(tlsdev::kNoiseThreads), curve_lds, main_stream(ctx), a);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) {
            hipLaunchKernelGGL(width_kernel, dim3((unsigned)W, (unsigned)rows), dim3(tlsdev::kNoiseThreads), width_lds, main_stream(ctx), a);
            e = hipGetLastError();
        }
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(main_stream(ctx));
            return fail(ctx, TLS_E_HIP, std::string("noise profile launch: ") + hipGetErrorString(e));
        }
        ctx->last_kernel = "tls_noise_profile";
        TLS_HIP(ctx, hipMemcpyAsync(out_curves + k0, d_records, rows * tlsdev::kNoiseWords * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        TLS_HIP(ctx, hipMemcpyAsync(out_count + (size_t)k0 * W, d_count, rows * W * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        TLS_HIP(ctx, hipMemcpyAsync(out_robust + (size_t)k0 * W, d_robust, rows * W * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        TLS_HIP(ctx, hipMemcpyAsync(out_rms + (size_t)k0 * W, d_rms, rows * W * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));       // (the next slab overwrites the device buffers; w32 lives until here)
    }
    return TLS_OK;
}

// ---- decorrelation (tls_decorrelate.hip.h, DESIGN.md "Decorrelation"): one workgroup a (curve, segment); the shared columns
// and the segment bounds go up once a call, the rows slab by slab
static_assert(sizeof(tls_decor_fit) == tlsdev::kDecorWords * 8, "tls_decor_fit is the kernel's record");
static_assert(TLS_DECOR_MAX_TERMS == tlsdev::kDecorMaxTerms && TLS_DECOR_MAX_ITER == tlsdev::kDecorMaxIter &&
              TLS_DECOR_LDS_POINTS == tlsdev::kDecorLdsPoints, "the header's limits");

int tls_decorrelate(tls_ctx* ctx, const double* y, const double* dy, const uint8_t* mask, int64_t n, int64_t n_curves,
                    const double* shared, int64_t n_shared, const double* own, int64_t n_own, const int64_t* segments,
                    int64_t n_segments, double ridge, int64_t n_iter, double sigma_upper, double sigma_lower, double* out_flat,
                    double* out_trend, tls_decor_fit* out_fit, double* out_coef, double* out_mean, double* out_scale) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (n < 1 || n > 100000000) return fail(ctx, TLS_E_ARG, "decorrelation: n out of range [1, 1e8]");
    if (n_curves < 0) return fail(ctx, TLS_E_ARG, "decorrelation: n_curves < 0");
    if (n_shared < 0 || n_own < 0 || n_shared + n_own < 1 || n_shared > TLS_DECOR_MAX_TERMS || n_own > TLS_DECOR_MAX_TERMS ||
        n_shared + n_own > TLS_DECOR_MAX_TERMS)
        return fail(ctx, TLS_E_ARG, "decorrelation: n_shared + n_own out of range [1, 16]");
    if (n_segments < 1 || n_segments > n) return fail(ctx, TLS_E_ARG, "decorrelation: n_segments out of range [1, n]");
    if (!segments) return fail(ctx, TLS_E_ARG, "null argument");
    for (int64_t s = 0; s <= n_segments; ++s)
        if ((s == 0 && segments[0] != 0) || (s > 0 && segments[s] <= segments[s - 1]) || (s == n_segments && segments[s] != n))
            return fail(ctx, TLS_E_ARG, "decorrelation: segments must ascend strictly from 0 to n");
    if (!(std::isfinite(ridge) && ridge >= 0.0)) return fail(ctx, TLS_E_ARG, "decorrelation: ridge must be finite and >= 0");
    if (n_iter < 0 || n_iter > TLS_DECOR_MAX_ITER) return fail(ctx, TLS_E_ARG, "decorrelation: n_iter out of range [0, 16]");
    if (!(sigma_upper > 0.0) || !(sigma_lower > 0.0)) return fail(ctx, TLS_E_ARG, "decorrelation: the sigmas must be > 0");
    if (n_curves == 0) return TLS_OK;
    if (!y || !out_flat || !out_fit || (n_shared && !shared) || (n_own && !own)) return fail(ctx, TLS_E_ARG, "null argument");
    const size_t nn = (size_t)n, m = (size_t)(n_shared + n_own), S = (size_t)n_segments;
    if ((uint64_t)n_curves > (uint64_t)(SIZE_MAX / 8) / ((uint64_t)n * (uint64_t)(n_own + 1)))
        return fail(ctx, TLS_E_ARG, "decorrelation: rows too large");
    for (size_t q = 0; q < (size_t)n_curves * nn; ++q) {
        if (!(std::isfinite(y[q]) && y[q] > 0.0))
            return fail(ctx, TLS_E_ARG, "decorrelation: row " + std::to_string(q / nn) + " has a non-finite or non-positive value");
        if (dy && !(std::isfinite(dy[q]) && dy[q] > 0.0))
            return fail(ctx, TLS_E_ARG, "decorrelation: dy of row " + std::to_string(q / nn) + " has a non-finite or non-positive value");
    }
    for (size_t q = 0; q < (size_t)n_shared * nn; ++q)
        if (!std::isfinite(shared[q])) return fail(ctx, TLS_E_ARG, "decorrelation: shared has a non-finite value");
    for (size_t q = 0; q < (size_t)n_curves * (size_t)n_own * nn; ++q)
        if (!std::isfinite(own[q])) return fail(ctx, TLS_E_ARG, "decorrelation: own has a non-finite value");
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    int64_t longest = 0;
    for (int64_t s = 0; s < n_segments; ++s) longest = std::max(longest, segments[s + 1] - segments[s]);
    const size_t member_words = longest > tlsdev::kDecorLdsPoints ? (size_t)((longest + 31) / 32) : 0;
    // curves per launch: at most 256 MB of rows and columns, and the grid within 2^31 - 1 workgroups
    const size_t row_bytes = nn * (8 * (3 + (dy ? 1 : 0) + (size_t)n_own) + (mask ? 1 : 0));
    const int64_t slab = std::max<int64_t>(1, std::min<int64_t>({n_curves, (int64_t)((256u << 20) / row_bytes), (int64_t)(0x7fffffff / S)}));
    const size_t B = (size_t)slab;
    double *d_shared, *d_y, *d_dy, *d_own, *d_flat, *d_trend, *d_record, *d_coef, *d_mean, *d_scale;
    long long* d_segments;
    unsigned int* d_members;
    unsigned char* d_mask;
    Arena L;
    L.add(d_shared, (size_t)n_shared * nn);  L.add(d_segments, S + 1);          // of the call
    L.add(d_y, B * nn);                                                          // of one slab, from here on
    L.add(d_dy, dy ? B * nn : 0);  L.add(d_own, B * (size_t)n_own * nn);  L.add(d_flat, B * nn);  L.add(d_trend, B * nn);
    L.add(d_record, B * S * tlsdev::kDecorWords);  L.add(d_coef, B * S * m);  L.add(d_mean, B * S * m);  L.add(d_scale, B * S * m);
    L.add(d_members, B * S * member_words);  L.add(d_mask, mask ? B * nn : 0);
    TLS_HIP(ctx, L.bind(ctx->d_decor));
    std::vector<long long> seg(S + 1);
    for (size_t s = 0; s <= S; ++s) seg[s] = (long long)segments[s];
    if (n_shared) TLS_HIP(ctx, hipMemcpyAsync(d_shared, shared, (size_t)n_shared * nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_segments, seg.data(), (S + 1) * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    tlsdev::DecorArgs a;
    a.y = d_y; a.dy = d_dy; a.mask = d_mask; a.shared = d_shared; a.own = d_own; a.segments = d_segments;
    a.flat = d_flat; a.trend = d_trend; a.record = d_record; a.coef = d_coef; a.mean = d_mean; a.scale = d_scale;
    a.members = d_members; a.n = (long long)n; a.member_words = (long long)member_words;
    a.ridge = ridge; a.sigma_upper = sigma_upper; a.sigma_lower = sigma_lower;
    a.n_shared = (int)n_shared; a.n_own = (int)n_own; a.S = (int)n_segments; a.n_iter = (int)n_iter;
    for (int64_t k0 = 0; k0 < n_curves; k0 += slab) {
        const size_t rows = (size_t)std::min<int64_t>(slab, n_curves - k0), at = (size_t)k0;
        TLS_HIP(ctx, hipMemcpyAsync(d_y, y + at * nn, rows * nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
        if (dy) TLS_HIP(ctx, hipMemcpyAsync(d_dy, dy + at * nn, rows * nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
        if (mask) TLS_HIP(ctx, hipMemcpyAsync(d_mask, mask + at * nn, rows * nn, hipMemcpyHostToDevice, main_stream(ctx)));
        if (n_own) TLS_HIP(ctx, hipMemcpyAsync(d_own, own + at * (size_t)n_own * nn, rows * (size_t)n_own * nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
        hipLaunchKernelGGL(tlsdev::tls_decorrelate_kernel, dim3((unsigned)(rows * S)), dim3(tlsdev::kDecorThreads), 0, main_stream(ctx), a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(main_stream(ctx));
            return fail(ctx, TLS_E_HIP, std::string("decorrelation launch: ") + hipGetErrorString(e));
        }
        ctx->last_kernel = "tls_decorrelate";
        TLS_HIP(ctx, hipMemcpyAsync(out_flat + at * nn, d_flat, rows * nn * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        if (out_trend) TLS_HIP(ctx, hipMemcpyAsync(out_trend + at * nn, d_trend, rows * nn * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        TLS_HIP(ctx, hipMemcpyAsync(out_fit + at * S, d_record, rows * S * tlsdev::kDecorWords * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        if (out_coef) TLS_HIP(ctx, hipMemcpyAsync(out_coef + at * S * m, d_coef, rows * S * m * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        if (out_mean) TLS_HIP(ctx, hipMemcpyAsync(out_mean + at * S * m, d_mean, rows * S * m * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        if (out_scale) TLS_HIP(ctx, hipMemcpyAsync(out_scale + at * S * m, d_scale, rows * S * m * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));       // (the next slab overwrites the device buffers; seg lives until here)
    }
    return TLS_OK;
}

// ---- cleaning (tls_clean.hip.h, DESIGN.md "Cleaning"): flags, rounds of a robust clip, repair.  The host forms the segments
// and (for a sliding centre) the biweight's windows and tiles once a call; a round is the tile pass (a sliding centre only) and
// the per-row kernel, and the host reads one count a round: the rows still running.
static_assert(sizeof(tls_clean_record) == tlsdev::kCleanWords * 8, "the header's record is the kernels'");
static_assert(TLS_CLEAN_MAX_ITER == tlsdev::kCleanMaxIter && TLS_CLEAN_LDS_POINTS == tlsdev::kNoiseLdsPoints, "the header's limits");
static_assert(tlsdev::clean_row_lds_bytes(tlsdev::kNoiseLdsPoints, true) <= 160 * 1024, "the LDS of a workgroup");
static_assert(tlsdev::clean_tile_lds_bytes(tlsdev::kDetrendMaxSpan, tlsdev::kDetrendMaxSpan) <= 160 * 1024, "the LDS of a workgroup");

int tls_clean_rows(tls_ctx* ctx, const double* t, const double* y, const uint8_t* bad, int64_t n, int64_t n_rows,
                   double window_length, double break_tolerance, double sigma_upper, double sigma_lower, int64_t max_run,
                   int64_t n_iter, int64_t min_points, double* out_rows, uint8_t* out_flags, tls_clean_record* out_records) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (n < 1 || n > 100000000) return fail(ctx, TLS_E_ARG, "cleaning: n out of range [1, 1e8]");
    if (n_rows < 0) return fail(ctx, TLS_E_ARG, "cleaning: n_rows < 0");
    if (!(std::isfinite(window_length) && window_length >= 0.0))
        return fail(ctx, TLS_E_ARG, "cleaning: window_length must be finite and > 0, or 0 for the row's median");
    if (!(break_tolerance > 0.0)) return fail(ctx, TLS_E_ARG, "cleaning: break_tolerance must be > 0");
    if (!(sigma_upper > 0.0) || !(sigma_lower > 0.0)) return fail(ctx, TLS_E_ARG, "cleaning: the sigmas must be > 0");
    if (max_run < 1) return fail(ctx, TLS_E_ARG, "cleaning: max_run must be >= 1");
    if (n_iter < 0 || n_iter > TLS_CLEAN_MAX_ITER) return fail(ctx, TLS_E_ARG, "cleaning: n_iter out of range [0, 16]");
    if (min_points < 1 || min_points > INT32_MAX) return fail(ctx, TLS_E_ARG, "cleaning: min_points must be >= 1");
    if (!t) return fail(ctx, TLS_E_ARG, "null argument");
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(t[i]) || (i > 0 && !(t[i] >= t[i - 1])))
            return fail(ctx, TLS_E_ARG, "cleaning: t must be finite and non-decreasing (index " + std::to_string(i) + ")");
    const size_t nn = (size_t)n;
    const bool sliding = window_length > 0.0;
    // the segments, and the biweight's windows: [lo_i, hi_i) inside i's segment, |t[j] - t[i]| <= window_length / 2
    std::vector<int> seg(nn), lo, hi;
    for (int64_t i = 0, s = 0; i < n; ++i) {
        if (i > 0 && t[i] - t[i - 1] > break_tolerance) ++s;
        seg[(size_t)i] = (int)s;
    }
    int64_t wmax = 0;
    if (sliding) {
        lo.resize(nn);
        hi.resize(nn);
        const double half = 0.5 * window_length;
        int64_t start = 0, wlo = 0, whi = 0;
        for (int64_t i = 0; i < n; ++i) {
            if (i > 0 && t[i] - t[i - 1] > break_tolerance) start = i;
            wlo = std::max(wlo, start);
            while (std::fabs(t[wlo] - t[i]) > half) ++wlo;
            whi = std::max(whi, i + 1);
            while (whi < n && !(t[whi] - t[whi - 1] > break_tolerance) && std::fabs(t[whi] - t[i]) <= half) ++whi;
            lo[(size_t)i] = (int)wlo;
            hi[(size_t)i] = (int)whi;
            wmax = std::max(wmax, whi - wlo);
        }
        if (wmax > TLS_BIWEIGHT_MAX_WINDOW)
            return fail(ctx, TLS_E_ARG, "cleaning: a window holds " + std::to_string(wmax) + " points, more than " +
                                            std::to_string(TLS_BIWEIGHT_MAX_WINDOW));
    }
    if (n_rows == 0) return TLS_OK;
    if (!y || !out_rows || !out_records) return fail(ctx, TLS_E_ARG, "null argument");
    if ((uint64_t)n_rows > (uint64_t)(SIZE_MAX / 32) / (uint64_t)n) return fail(ctx, TLS_E_ARG, "cleaning: rows too large");
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    const bool rounds_wanted = n_iter > 0 && !(std::isinf(sigma_upper) && std::isinf(sigma_lower));
    const bool lds = n <= tlsdev::kNoiseLdsPoints;
    // rows per launch: the grid's limit, and at most 256 MB of rows, residuals, flags and codes
    const int64_t slab = std::max<int64_t>(1, std::min<int64_t>({n_rows, (int64_t)65535, (int64_t)((256u << 20) / (27 * nn))}));
    const size_t B = (size_t)slab;
    double *d_t, *d_y, *d_r, *d_out, *d_records;
    unsigned long long* d_counts;
    int *d_seg, *d_lo, *d_hi;
    unsigned int* d_run;
    unsigned char *d_bad, *d_flags, *d_code;
    Arena L;
    L.add(d_t, nn);  L.add(d_counts, (size_t)TLS_CLEAN_MAX_ITER);                                           // of the call
    L.add(d_y, B * nn);  L.add(d_r, B * nn);  L.add(d_out, B * nn);  L.add(d_records, B * tlsdev::kCleanWords);   // of one slab, from here on
    L.add(d_seg, nn);  L.add(d_lo, sliding ? nn : 0);  L.add(d_hi, sliding ? nn : 0);  L.add(d_run, B);
    L.add(d_bad, bad ? B * nn : 0);  L.add(d_flags, B * nn);  L.add(d_code, lds ? 0 : B * nn);
    TLS_HIP(ctx, L.bind(ctx->d_clean));
    TLS_HIP(ctx, hipMemcpyAsync(d_t, t, nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_seg, seg.data(), nn * sizeof(int), hipMemcpyHostToDevice, main_stream(ctx)));
    int T = 0, P = 0, smax = 0;
    size_t tile_lds = 0;
    if (sliding) {
        TLS_HIP(ctx, hipMemcpyAsync(d_lo, lo.data(), nn * sizeof(int), hipMemcpyHostToDevice, main_stream(ctx)));
        TLS_HIP(ctx, hipMemcpyAsync(d_hi, hi.data(), nn * sizeof(int), hipMemcpyHostToDevice, main_stream(ctx)));
        biweight_plan(lo, hi, wmax, &T, &P, &smax);
        tile_lds = tlsdev::clean_tile_lds_bytes(P, smax);
        TLS_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(tlsdev::tls_clean_tile), hipFuncAttributeMaxDynamicSharedMemorySize, (int)tile_lds));
    }
    auto row_kernel = lds ? tlsdev::tls_clean_row_kernel<true> : tlsdev::tls_clean_row_kernel<false>;
    const size_t row_lds = tlsdev::clean_row_lds_bytes((int)n, lds);
    TLS_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(row_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)row_lds));
    tlsdev::CleanArgs a;
    a.t = d_t; a.seg = d_seg; a.y = d_y; a.bad = d_bad; a.flags = d_flags; a.r = d_r; a.code = d_code; a.out = d_out;
    a.records = d_records; a.run = d_run; a.counts = d_counts; a.check = nullptr; a.lo = sliding ? d_lo : nullptr;
    a.hi = sliding ? d_hi : nullptr; a.sigma_upper = sigma_upper; a.sigma_lower = sigma_lower; a.max_run = (long long)max_run;
    a.n = (long long)n; a.n_iter = (int)n_iter; a.min_points = (int)min_points; a.round = 0; a.rounds_wanted = rounds_wanted ? 1 : 0;
    a.tile = T; a.span = P; a.smax = smax;
#ifdef TLS_DEBUG_CHECKS
    if (int rc = ensure_check_counters(ctx)) return rc;
    a.check = ctx->d_check.ptr;
#endif
    auto launched = [&](const char* what) -> int {
        const hipError_t e = hipGetLastError();
        if (e == hipSuccess) return TLS_OK;
        (void)hipStreamSynchronize(main_stream(ctx));
        return fail(ctx, TLS_E_HIP, std::string("cleaning ") + what + " launch: " + hipGetErrorString(e));
    };
    const unsigned tiles = sliding ? (unsigned)((n + T - 1) / T) : 0u;
    for (int64_t k0 = 0; k0 < n_rows; k0 += slab) {
        const size_t rows = (size_t)std::min<int64_t>(slab, n_rows - k0), at = (size_t)k0 * nn;
        TLS_HIP(ctx, hipMemcpyAsync(d_y, y + at, rows * nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
        if (bad) TLS_HIP(ctx, hipMemcpyAsync(d_bad, bad + at, rows * nn, hipMemcpyHostToDevice, main_stream(ctx)));
        TLS_HIP(ctx, hipMemsetAsync(d_counts, 0, TLS_CLEAN_MAX_ITER * 8, main_stream(ctx)));
        a.count = (long long)rows * (long long)n;
        const unsigned blocks = (unsigned)std::min<long long>((a.count + tlsdev::kDetrendThreads - 1) / tlsdev::kDetrendThreads, 65536);
        hipLaunchKernelGGL(tlsdev::tls_clean_init, dim3(blocks), dim3(tlsdev::kDetrendThreads), 0, main_stream(ctx), a);
        if (int rc = launched("init")) return rc;
        for (int64_t k = 0; rounds_wanted && k < n_iter; ++k) {
            a.round = (int)k;
            if (sliding) {
                hipLaunchKernelGGL(tlsdev::tls_clean_tile, dim3(tiles, (unsigned)rows), dim3(tlsdev::kDetrendThreads), tile_lds, main_stream(ctx), a);
                if (int rc = launched("tile")) return rc;
            }
            hipLaunchKernelGGL(row_kernel, dim3((unsigned)rows), dim3(tlsdev::kNoiseThreads), row_lds, main_stream(ctx), a);
            if (int rc = launched("row")) return rc;
            if (k + 1 < n_iter) {
                unsigned long long going = 0;
                TLS_HIP(ctx, hipMemcpyAsync(&going, d_counts + k, 8, hipMemcpyDeviceToHost, main_stream(ctx)));
                TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));
                if (going == 0) break;
            }
        }
        hipLaunchKernelGGL(tlsdev::tls_clean_repair_kernel, dim3((unsigned)rows), dim3(tlsdev::kNoiseThreads), 0, main_stream(ctx), a);
        if (int rc = launched("repair")) return rc;
        ctx->last_kernel = "tls_clean_rows";
        TLS_HIP(ctx, hipMemcpyAsync(out_rows + at, d_out, rows * nn * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        if (out_flags) TLS_HIP(ctx, hipMemcpyAsync(out_flags + at, d_flags, rows * nn, hipMemcpyDeviceToHost, main_stream(ctx)));
        TLS_HIP(ctx, hipMemcpyAsync(out_records + k0, d_records, rows * tlsdev::kCleanWords * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));       // (the next slab overwrites the device buffers; seg, lo and hi live until here)
    }
    return TLS_OK;
}

// ---- spline detrending (tls_spline.hip.h, DESIGN.md "Spline detrending"): one workgroup a (segment, spacing, curve).  The
// host forms the segments of t and q and h of every (spacing, segment); with several spacings a records-only launch, the pick
// and a launch at the picked spacing follow one another on the stream, with one spacing the fit and the pick.
static_assert(sizeof(tls_spline_segment) == tlsdev::kSplineSegWords * 8 && sizeof(tls_spline_curve) == tlsdev::kSplineCurveWords * 8,
              "the header's records are the kernels'");
static_assert(TLS_SPLINE_MAX_SPACINGS == tlsdev::kSplineMaxSpacings && TLS_SPLINE_MAX_ITER == tlsdev::kSplineMaxIter &&
              TLS_SPLINE_MAX_COEF == tlsdev::kSplineMaxCoef && TLS_SPLINE_LDS_POINTS == tlsdev::kSplineLdsPoints,
              "the header's limits");
static_assert(tlsdev::spline_lds_bytes(tlsdev::kSplineMaxCoef, tlsdev::kSplineLdsPoints, true) <= 160 * 1024, "the LDS of a workgroup");

int tls_spline_detrend(tls_ctx* ctx, const double* t, const double* y, const double* dy, const uint8_t* mask, int64_t n,
                       int64_t n_rows, const double* spacings, int64_t n_spacings, double break_tolerance, double penalty,
                       int64_t n_iter, double sigma_upper, double sigma_lower, double* out_flat, double* out_trend,
                       tls_spline_segment* out_segment_records, tls_spline_curve* out_curve_records) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (n < 1 || n > 100000000) return fail(ctx, TLS_E_ARG, "spline detrending: n out of range [1, 1e8]");
    if (n_rows < 0) return fail(ctx, TLS_E_ARG, "spline detrending: n_rows < 0");
    if (n_spacings < 1 || n_spacings > TLS_SPLINE_MAX_SPACINGS) return fail(ctx, TLS_E_ARG, "spline detrending: n_spacings out of range [1, 16]");
    if (!t || !spacings) return fail(ctx, TLS_E_ARG, "null argument");
    for (int64_t s = 0; s < n_spacings; ++s)
        if (!(std::isfinite(spacings[s]) && spacings[s] > 0.0)) return fail(ctx, TLS_E_ARG, "spline detrending: every knot spacing must be finite and > 0");
    if (!(break_tolerance > 0.0)) return fail(ctx, TLS_E_ARG, "spline detrending: break_tolerance must be > 0");
    if (!(std::isfinite(penalty) && penalty >= 0.0)) return fail(ctx, TLS_E_ARG, "spline detrending: penalty must be finite and >= 0");
    if (n_iter < 0 || n_iter > TLS_SPLINE_MAX_ITER) return fail(ctx, TLS_E_ARG, "spline detrending: n_iter out of range [0, 16]");
    if (!(sigma_upper > 0.0) || !(sigma_lower > 0.0)) return fail(ctx, TLS_E_ARG, "spline detrending: the sigmas must be > 0");
    const size_t nn = (size_t)n, S = (size_t)n_spacings;
    for (size_t i = 0; i < nn; ++i)
        if (!std::isfinite(t[i]) || (i > 0 && t[i] < t[i - 1])) return fail(ctx, TLS_E_ARG, "spline detrending: t must be finite and non-decreasing");
    // the segments, and q and h of every (spacing, segment)
    std::vector<long long> seg(1, 0);
    for (size_t i = 1; i < nn; ++i)
        if (t[i] - t[i - 1] > break_tolerance) seg.push_back((long long)i);
    seg.push_back((long long)n);
    const size_t G = seg.size() - 1;
    std::vector<int> qs(S * G);
    std::vector<double> hs(S * G);
    int m_max = 0;
    long long longest = 0;
    for (size_t g = 0; g < G; ++g) {
        longest = std::max(longest, seg[g + 1] - seg[g]);
        const double T = t[seg[g + 1] - 1] - t[seg[g]];
        for (size_t s = 0; s < S; ++s) {
            int q = 0;
            double h = (double)NAN;
            if (T != 0.0) {
                const double want = std::ceil(T / spacings[s]);
                if (!(want <= (double)(TLS_SPLINE_MAX_COEF - 3)))
                    return fail(ctx, TLS_E_ARG, "spline detrending: a segment has more than " + std::to_string(TLS_SPLINE_MAX_COEF) + " coefficients");
                q = std::max(1, (int)want);
                h = T / (double)q;
                m_max = std::max(m_max, q + 3);
            }
            qs[s * G + g] = q;
            hs[s * G + g] = h;
        }
    }
    if (n_rows == 0) return TLS_OK;
    if (!y || !out_flat || !out_segment_records || !out_curve_records) return fail(ctx, TLS_E_ARG, "null argument");
    if ((uint64_t)n_rows > (uint64_t)(SIZE_MAX / 8) / ((uint64_t)n * (uint64_t)(S + 2)))
        return fail(ctx, TLS_E_ARG, "spline detrending: rows too large");
    for (size_t k = 0; k < (size_t)n_rows * nn; ++k) {
        if (!(std::isfinite(y[k]) && y[k] > 0.0))
            return fail(ctx, TLS_E_ARG, "spline detrending: row " + std::to_string(k / nn) + " has a non-finite or non-positive value");
        if (dy && !(std::isfinite(dy[k]) && dy[k] > 0.0))
            return fail(ctx, TLS_E_ARG, "spline detrending: dy of row " + std::to_string(k / nn) + " has a non-finite or non-positive value");
    }
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    const bool lds = longest <= tlsdev::kSplineLdsPoints;
    const int mcap = std::max(4, (m_max + 1) & ~1), pcap = lds ? (int)((longest + 1) & ~1LL) : 0;
    const size_t lds_bytes = tlsdev::spline_lds_bytes(mcap, pcap, lds);
    // curves per launch: gridDim.z within its limit, at most 256 MB of rows and at most 256 MB of the long segments' scratch
    const size_t row_bytes = nn * (8 * (3 + (dy ? 1 : 0)) + (mask ? 1 : 0)), scratch_bytes = lds ? 0 : nn * 17 * S;
    int64_t slab = std::min<int64_t>({n_rows, (int64_t)65535, (int64_t)((256u << 20) / row_bytes)});
    if (!lds) slab = std::min<int64_t>(slab, (int64_t)((256u << 20) / scratch_bytes));
    slab = std::max<int64_t>(1, slab);
    const size_t B = (size_t)slab;
    double *d_t, *d_h, *d_y, *d_dy, *d_flat, *d_trend, *d_tried, *d_records, *d_curves, *d_gw, *d_gr;
    long long* d_seg;
    int* d_q;
    unsigned char *d_mask, *d_gmember;
    Arena L;
    L.add(d_t, nn);  L.add(d_seg, G + 1);  L.add(d_h, S * G);  L.add(d_q, S * G);                     // of the call
    L.add(d_y, B * nn);  L.add(d_dy, dy ? B * nn : 0);  L.add(d_flat, B * nn);  L.add(d_trend, B * nn);       // of one slab, from here on
    L.add(d_tried, S > 1 ? B * S * G * tlsdev::kSplineSegWords : 0);  L.add(d_records, B * G * tlsdev::kSplineSegWords);
    L.add(d_curves, B * tlsdev::kSplineCurveWords);
    L.add(d_gw, lds ? 0 : B * S * nn);  L.add(d_gr, lds ? 0 : B * S * nn);                                  // the long segments' scratch
    L.add(d_mask, mask ? B * nn : 0);  L.add(d_gmember, lds ? 0 : B * S * nn);
    TLS_HIP(ctx, L.bind(ctx->d_spline));
    TLS_HIP(ctx, hipMemcpyAsync(d_t, t, nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_seg, seg.data(), (G + 1) * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_h, hs.data(), S * G * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(d_q, qs.data(), S * G * 4, hipMemcpyHostToDevice, main_stream(ctx)));
    auto fit_kernel = lds ? tlsdev::tls_spline_fit_kernel<true> : tlsdev::tls_spline_fit_kernel<false>;
    TLS_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(fit_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    tlsdev::SplineArgs a;
    a.t = d_t; a.y = d_y; a.dy = d_dy; a.mask = d_mask; a.seg = d_seg; a.q = d_q; a.h = d_h;
    a.gw = d_gw; a.gr = d_gr; a.gmember = d_gmember; a.check = nullptr;
    a.penalty = penalty; a.sigma_upper = sigma_upper; a.sigma_lower = sigma_lower;
    a.n = (long long)n; a.G = (int)G; a.n_iter = (int)n_iter; a.mcap = mcap; a.pcap = pcap;
    tlsdev::SplinePickArgs p;
    p.t = d_t; p.y = d_y; p.mask = d_mask; p.curves = d_curves; p.check = nullptr;
    p.break_tolerance = break_tolerance; p.n = (int)n; p.G = (int)G; p.S = (int)S;
#ifdef TLS_DEBUG_CHECKS
    if (int rc = ensure_check_counters(ctx)) return rc;
    a.check = ctx->d_check.ptr;
    p.check = ctx->d_check.ptr;
#endif
    for (int64_t k0 = 0; k0 < n_rows; k0 += slab) {
        const size_t rows = (size_t)std::min<int64_t>(slab, n_rows - k0), at = (size_t)k0;
        TLS_HIP(ctx, hipMemcpyAsync(d_y, y + at * nn, rows * nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
        if (dy) TLS_HIP(ctx, hipMemcpyAsync(d_dy, dy + at * nn, rows * nn * 8, hipMemcpyHostToDevice, main_stream(ctx)));
        if (mask) TLS_HIP(ctx, hipMemcpyAsync(d_mask, mask + at * nn, rows * nn, hipMemcpyHostToDevice, main_stream(ctx)));
        hipError_t e = hipSuccess;
        if (S > 1) {                                 // every spacing, the records alone; then the pick
            a.choice = nullptr; a.flat = nullptr; a.trend = nullptr; a.records = d_tried; a.S = (int)S;
            hipLaunchKernelGGL(fit_kernel, dim3((unsigned)G, (unsigned)S, (unsigned)rows), dim3(tlsdev::kSplineThreads), lds_bytes, main_stream(ctx), a);
            e = hipGetLastError();
            if (e == hipSuccess) {
                p.records = d_tried;
                hipLaunchKernelGGL(tlsdev::tls_spline_pick_kernel, dim3((unsigned)rows), dim3(tlsdev::kSplineThreads), 0, main_stream(ctx), p);
                e = hipGetLastError();
            }
        }
        if (e == hipSuccess) {                       // the fit that goes out: at the picked spacing, or at the only one
            a.choice = S > 1 ? d_curves : nullptr; a.flat = d_flat; a.trend = d_trend; a.records = d_records; a.S = 1;
            hipLaunchKernelGGL(fit_kernel, dim3((unsigned)G, 1u, (unsigned)rows), dim3(tlsdev::kSplineThreads), lds_bytes, main_stream(ctx), a);
            e = hipGetLastError();
        }
        if (e == hipSuccess && S == 1) {
            p.records = d_records;
            hipLaunchKernelGGL(tlsdev::tls_spline_pick_kernel, dim3((unsigned)rows), dim3(tlsdev::kSplineThreads), 0, main_stream(ctx), p);
            e = hipGetLastError();
        }
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(main_stream(ctx));
            return fail(ctx, TLS_E_HIP, std::string("spline detrending launch: ") + hipGetErrorString(e));
        }
        ctx->last_kernel = "tls_spline_detrend";
        TLS_HIP(ctx, hipMemcpyAsync(out_flat + at * nn, d_flat, rows * nn * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        if (out_trend) TLS_HIP(ctx, hipMemcpyAsync(out_trend + at * nn, d_trend, rows * nn * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        TLS_HIP(ctx, hipMemcpyAsync(out_segment_records + at * G, d_records, rows * G * tlsdev::kSplineSegWords * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        TLS_HIP(ctx, hipMemcpyAsync(out_curve_records + at, d_curves, rows * tlsdev::kSplineCurveWords * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));       // (the next slab overwrites the device buffers; seg, qs and hs live until here)
    }
    return TLS_OK;
}

int tls_find_peaks(tls_ctx* ctx, const double* power, const double* chi2, const int64_t* row, const double* depth,
                   int64_t n_rows, int64_t n_periods, const double* periods, int64_t k, double min_separation,
                   const double* ratios, int64_t n_ratios, double min_power, tls_peak* out_peaks, int64_t* out_n_peaks) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (n_rows < 0) return fail(ctx, TLS_E_ARG, "peaks: n_rows < 0");
    PeaksRequest pk;
    pk.k = k; pk.sep = min_separation; pk.ratios = ratios; pk.n_ratios = n_ratios; pk.min_power = min_power;
    pk.out = out_peaks; pk.out_n = out_n_peaks;
    int rc = check_peaks_request(ctx, pk, n_periods);
    if (rc || n_rows == 0) return rc;
    if (!power || !periods || !out_peaks || !out_n_peaks) return fail(ctx, TLS_E_ARG, "null argument");
    if ((uint64_t)n_rows > (uint64_t)(SIZE_MAX / 64) / (uint64_t)n_periods) return fail(ctx, TLS_E_ARG, "peaks: rows too large");
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t np = (size_t)n_periods, words = pk.words();
    const size_t parts = 1 + (chi2 ? 1 : 0) + (row ? 1 : 0) + (depth ? 1 : 0);
    // rows per launch: at most 256 MB of rows (as the detrending slabs)
    const int64_t slab = std::max<int64_t>(1, std::min<int64_t>({n_rows, (int64_t)65535, (int64_t)((256u << 20) / (8 * np * parts))}));
    double *d_periods, *d_out, *d_power, *d_chi2, *d_depth;
    long long* d_row;
    Arena L;
    L.add(d_periods, np);  L.add(d_out, (size_t)slab * words);   // the records of one slab
    L.add(d_power, (size_t)slab * np);              // ... and its rows
    L.add(d_chi2, chi2 ? (size_t)slab * np : 0);  L.add(d_depth, depth ? (size_t)slab * np : 0);
    L.add(d_row, row ? (size_t)slab * np : 0);
    TLS_HIP(ctx, L.bind(ctx->d_peaks));
    if ((rc = reserve_peak_mask(ctx, slab, n_periods))) return rc;
    std::vector<double> h((size_t)slab * words);
    TLS_HIP(ctx, hipMemcpyAsync(d_periods, periods, np * 8, hipMemcpyHostToDevice, main_stream(ctx)));
    for (int64_t k0 = 0; k0 < n_rows; k0 += slab) {
        const int64_t rows = std::min<int64_t>(slab, n_rows - k0);
        const size_t bytes = (size_t)rows * np * 8, at = (size_t)k0 * np;
        TLS_HIP(ctx, hipMemcpyAsync(d_power, power + at, bytes, hipMemcpyHostToDevice, main_stream(ctx)));
        if (chi2) TLS_HIP(ctx, hipMemcpyAsync(d_chi2, chi2 + at, bytes, hipMemcpyHostToDevice, main_stream(ctx)));
        if (depth) TLS_HIP(ctx, hipMemcpyAsync(d_depth, depth + at, bytes, hipMemcpyHostToDevice, main_stream(ctx)));
        if (row) TLS_HIP(ctx, hipMemcpyAsync(d_row, row + at, bytes, hipMemcpyHostToDevice, main_stream(ctx)));
        if ((rc = enqueue_find_peaks(ctx, pk, rows, n_periods, d_power, np, d_periods, d_chi2, d_row, d_depth, nullptr, d_out))) {
            (void)hipStreamSynchronize(main_stream(ctx));
            return rc;
        }
        ctx->last_kernel = "tls_find_peaks";
        TLS_HIP(ctx, hipMemcpyAsync(h.data(), d_out, (size_t)rows * words * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        // (the next slab overwrites the device rows: the copies above have to be done first)
        TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));
        for (int64_t c = 0; c < rows; ++c) read_peaks(pk, h.data(), c, k0 + c);
    }
    return TLS_OK;
}

static int power_batch_impl(tls_ctx* ctx, const double* t, const double* y, const double* dy, int64_t n, int64_t n_curves,
                            const double* periods, int64_t n_periods, const tls_template* tmpl, const tls_params* params,
                            int64_t median_kernel, tls_power_summary* out_summary, double* out_chi2, int64_t* out_row,
                            double* out_depth, double* out_power, double* out_SR, double* out_power_raw,
                            const StatsRequest* sr, const ModelsRequest* mr, const PeaksRequest* pk, const PeakFitsRequest* pf,
                            const PhaseScanRequest* ps) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (n_curves < 0) return fail(ctx, TLS_E_ARG, "negative number of light curves");
    if (n_curves == 0) return TLS_OK;
    if (!t || !y || !dy || !periods || !tmpl || !params || !out_summary) return fail(ctx, TLS_E_ARG, "null argument");
    if (n_periods < 1) return fail(ctx, TLS_E_ARG, "tls_power_batch needs at least one period");
    if (median_kernel < 1 || median_kernel > 8000) return fail(ctx, TLS_E_ARG, "median kernel out of range [1, 8000]");
    if ((out_row == nullptr) != (out_chi2 == nullptr) || (out_depth == nullptr) != (out_chi2 == nullptr))
        return fail(ctx, TLS_E_ARG, "out_chi2, out_row and out_depth go together (all or none)");
    int rc = tls_prepare(ctx, t, y, dy, n, periods, n_periods, tmpl, params);   // the plan, from the first curve
    if (rc) return rc;
    const int64_t group = std::min<int64_t>(32, n_curves);              // (one light curve: the drop-in power() call)
    const size_t np = (size_t)n_periods, nn = (size_t)n;
    double t_min, t_max;
    time_range(t, n, t_min, t_max);
    // device buffers of one group: flux (weights), per-curve constants, search results, spectra, summaries, T0-fit inputs
    auto& sl = ctx->slot[0];
    if ((rc = reserve_batch_slot(ctx, sl, group, nn, np))) return rc;
    TLS_HIP(ctx, ctx->d_perm.reserve(perm_scratch_words(ctx, nn)));
    int64_t max_len = 1;
    for (int64_t r = 0; r < tmpl->n_rows; ++r) max_len = std::max(max_len, tmpl->length[r]);
    // (statistics requested: their records -- and the per-transit rows when asked for -- ride in the group's one copy out;
    // peaks requested: their records lie behind those and ride in it too)
    const size_t stats_out = !sr ? 0 : sr->out_per_transit ? sr->words() : (size_t)tlsdev::kTransitStats;
    const size_t peaks_out = pk ? pk->words() : 0;
    // (peak fits requested, with peaks only: T0, status and record of every peak, behind the peaks, in the same copy)
    const size_t fits_out = pf ? pf->words() : 0;
    // (phase scans requested, with peak fits only: one record a peak, behind the fits, in the same copy)
    const size_t scans_out = pf && ps ? (size_t)tlsdev::kPhaseWords * (size_t)pf->k : 0;
    PostSearchBufs pb;
    if ((rc = reserve_post_search(ctx, group, n_periods, n, max_len, pb, sr ? sr->words() : 0, peaks_out, stats_out, fits_out, scans_out))) return rc;
    const size_t spec_stride = pb.spec_stride;
    StatsBufs sb;
    if (sr && (rc = reserve_transit_stats(ctx, *sr, group, n, sb))) return rc;
    // (no statistics of the best pick: the peak fits still read the row durations and the root table on the device)
    if (pf && !sr && (rc = reserve_transit_stats(ctx, *pf->inputs, 0, n, sb))) return rc;
    PeakFitBufs fb;
    if (pf && (rc = reserve_peak_fits(ctx, group * pf->k, n, max_len, pf->inputs->max_epochs, fb))) return rc;
    if (pk && (rc = reserve_peak_mask(ctx, group, n_periods))) return rc;
    // (models requested: the folded light curve, the folded model and the padded model light curve of every curve, behind them)
    ModelsBufs mb;
    if (mr && (rc = reserve_transit_models(ctx, *mr, group, n, mb))) return rc;
    const size_t models_out = mr ? mb.out_stride : 0;
    // pinned staging: flux in; summaries, T0 and (on request) the per-period arrays out.  TWO sets (the device buffers are
    // one: the stream runs the groups in order): while the device works on group g the host forms group g + 1 in the other
    // set and enqueues it, THEN waits for g -- the device never waits for the host between two groups (round 6)
    const size_t arrays = (out_chi2 ? 3 : 0) + (out_power ? 1 : 0) + (out_SR ? 1 : 0) + (out_power_raw ? 1 : 0);
    const size_t out_doubles = (11 + stats_out + peaks_out + fits_out + scans_out + models_out) * (size_t)group + arrays * (size_t)group * np;
    if ((rc = reserve_batch_staging(ctx, group, nn, out_doubles))) return rc;
    const int64_t n_groups = (n_curves + group - 1) / group;
    ctx->batch_group_ms.assign((size_t)n_groups, 0.0);
    ctx->batch_group_wait_ms.assign((size_t)n_groups, 0.0);
    // host layout of a group's results (the same in both sets)
    struct OutLayout { double *sde, *pick, *T0, *stats, *peaks, *fits, *scans, *chi2, *power, *SR, *praw, *spec3, *models; };
    auto out_layout = [&](int64_t g) -> OutLayout {
        OutLayout o{};
        double* base = ctx->slot[g & 1].h_out;
        o.sde = base; o.pick = o.sde + 2 * (size_t)group; o.T0 = o.pick + 8 * (size_t)group;
        o.stats = o.T0 + group;                          // statistics records (and rows), on request
        o.peaks = o.stats + stats_out * (size_t)group;   // peak records, on request
        o.fits = o.peaks + peaks_out * (size_t)group;    // peak fits, on request
        o.scans = o.fits + fits_out * (size_t)group;     // phase scans, on request
        double* h_next = o.scans + scans_out * (size_t)group;   // chi2 | row | depth | power | SR | power_raw, on request
        if (out_chi2) { o.chi2 = h_next; h_next += 3 * (size_t)group * np; }
        if (out_power && out_SR && out_power_raw) { o.spec3 = h_next; h_next += 3 * (size_t)group * np; }
        else {
            if (out_power) { o.power = h_next; h_next += (size_t)group * np; }
            if (out_SR) { o.SR = h_next; h_next += (size_t)group * np; }
            if (out_power_raw) { o.praw = h_next; h_next += (size_t)group * np; }
        }
        if (mr) o.models = h_next;                       // the models' rows, on request
        return o;
    };
    // ---- group g formed in pinned set g & 1, then its device side, nothing waited for: flux up, search, spectra, pick,
    // final T0 fit, results down, an event behind them
    GroupState st;
    auto enqueue_group = [&](int64_t g) -> int {
        auto& hs = ctx->slot[g & 1];
        const int64_t c0 = g * group, gc = std::min(group, n_curves - c0);
        int rc2 = stage_group(ctx, hs, y, dy, n, c0, gc, group, st);
        if (rc2 || (rc2 = upload_group(ctx, sl, st, nn, main_stream(ctx))) || (rc2 = search_group(ctx, sl, st))) return rc2;
        // ---- spectra, pick and final T0 fit of every curve of the group
        rc2 = enqueue_post_search(ctx, pb, gc, sl.d_chi2.ptr, sl.d_row.ptr, sl.d_depth.ptr, sl.d_y.ptr, n, n_periods, median_kernel,
                                  t_min, t_max, params->T0_fit_margin);
        if (rc2) return rc2;
        // (the peaks read the detrended power and the pick's no-fit flag: nothing of the T0 fit)
        if (pk && (rc2 = enqueue_find_peaks(ctx, *pk, gc, n_periods, ctx->d_spec.ptr + 2 * np, spec_stride, ctx->d_periods.ptr,
                                            sl.d_chi2.ptr, sl.d_row.ptr, sl.d_depth.ptr, pb.pick, pb.peaks))) return rc2;
        if (sr && (rc2 = enqueue_transit_stats(ctx, pb, sb, *sr, gc, sl.d_y.ptr, n, n_periods, t_min, t_max))) return rc2;
        // (every peak's T0 fit and record, on the stage's own arrays: pick, T0 and statistics of the best pick stay as they are)
        if (pf && (rc2 = enqueue_peak_fits(ctx, fb, *pf, sb, gc, group, pb.peaks, pb.fits, sl.d_y.ptr, ctx->d_spec.ptr + 2 * np,
                                           spec_stride, n, n_periods, t_min, t_max, params->T0_fit_margin, 0,
                                           scans_out ? ps : nullptr, pb.scans))) return rc2;
        if (mr && (rc2 = enqueue_transit_models(ctx, pb, sb, *sr, *mr, mb, gc, sl.d_y.ptr, n, t_min, t_max))) return rc2;
        // (sde | pick | T0 [| statistics] [| peaks [| peak fits [| phase scans]]] lie side by side behind the spectra on the device: ONE copy, the host keeps the layout)
        const OutLayout o = out_layout(g);
        TLS_HIP(ctx, hipMemcpyAsync(o.sde, pb.sde, (11 + stats_out + peaks_out + fits_out + scans_out) * (size_t)group * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        if (out_chi2) {
            TLS_HIP(ctx, hipMemcpyAsync(o.chi2, sl.d_chi2.ptr, (size_t)gc * np * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
            TLS_HIP(ctx, hipMemcpyAsync(o.chi2 + (size_t)group * np, sl.d_row.ptr, (size_t)gc * np * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
            TLS_HIP(ctx, hipMemcpyAsync(o.chi2 + 2 * (size_t)group * np, sl.d_depth.ptr, (size_t)gc * np * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        }
        // (SR | power_raw | power lie side by side per light curve: all three asked for = one contiguous copy, else one strided copy each)
        auto fetch_spec = [&](double* host, size_t which) -> hipError_t {
            return hipMemcpy2DAsync(host, np * 8, ctx->d_spec.ptr + which * np, spec_stride * 8, np * 8, (size_t)gc, hipMemcpyDeviceToHost, main_stream(ctx));
        };
        if (o.spec3) TLS_HIP(ctx, hipMemcpyAsync(o.spec3, ctx->d_spec.ptr, (size_t)gc * spec_stride * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        if (o.power) TLS_HIP(ctx, fetch_spec(o.power, 2));
        if (o.SR) TLS_HIP(ctx, fetch_spec(o.SR, 0));
        if (o.praw) TLS_HIP(ctx, fetch_spec(o.praw, 1));
        if (o.models) TLS_HIP(ctx, hipMemcpyAsync(o.models, mb.out, (size_t)gc * mb.out_stride * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
        TLS_HIP(ctx, hipEventRecord(hs.ev_out, main_stream(ctx)));
        return TLS_OK;
    };
    // ---- results of group g: the ONE wait of the group, then the caller's arrays
    auto last_done = std::chrono::steady_clock::now();
    auto consume_group = [&](int64_t g) -> int {
        auto& hs = ctx->slot[g & 1];
        const int64_t c0 = g * group, gc = std::min(group, n_curves - c0);
        const auto wait_t0 = std::chrono::steady_clock::now();
        TLS_HIP(ctx, hipEventSynchronize(hs.ev_out));
        ctx->batch_group_wait_ms[(size_t)g] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wait_t0).count();
        const OutLayout o = out_layout(g);
        for (int64_t c = 0; c < gc; ++c) {
            const int rc2 = read_summary(ctx, o.sde, group, c, c0 + c, out_summary[c0 + c]);
            if (rc2) return rc2;
        }
        if (sr)
            for (int64_t c = 0; c < gc; ++c) {
                const int rc2 = read_transit_stats(ctx, *sr, o.stats, group, c, c0 + c, true);
                if (rc2) return rc2;
            }
        if (mr)
            for (int64_t c = 0; c < gc; ++c) {
                const int rc2 = read_transit_models(ctx, *mr, o.models, mb.out_stride, c, c0 + c, n);
                if (rc2) return rc2;
            }
        if (pk)
            for (int64_t c = 0; c < gc; ++c) read_peaks(*pk, o.peaks, c, c0 + c);
        if (pf)
            for (int64_t c = 0; c < gc; ++c) {
                const int rc2 = read_peak_fits(ctx, *pf, o.fits, group, c, c0 + c);
                if (rc2) return rc2;
            }
        if (scans_out)   // (fit f = c k + r of the group: curve c's k records lie side by side)
            for (int64_t c = 0; c < gc; ++c)
                std::memcpy(ps->out + (size_t)(c0 + c) * (size_t)pf->k, o.scans + (size_t)c * scans_out, scans_out * 8);
        if (out_chi2) {
            std::memcpy(out_chi2 + c0 * n_periods, o.chi2, (size_t)gc * np * 8);
            std::memcpy(out_row + c0 * n_periods, o.chi2 + (size_t)group * np, (size_t)gc * np * 8);
            std::memcpy(out_depth + c0 * n_periods, o.chi2 + 2 * (size_t)group * np, (size_t)gc * np * 8);
        }
        if (o.spec3) {
            for (int64_t c = 0; c < gc; ++c) {
                std::memcpy(out_SR + (c0 + c) * n_periods, o.spec3 + (size_t)c * spec_stride, np * 8);
                std::memcpy(out_power_raw + (c0 + c) * n_periods, o.spec3 + (size_t)c * spec_stride + np, np * 8);
                std::memcpy(out_power + (c0 + c) * n_periods, o.spec3 + (size_t)c * spec_stride + 2 * np, np * 8);
            }
        } else {
            if (out_power) std::memcpy(out_power + c0 * n_periods, o.power, (size_t)gc * np * 8);
            if (out_SR) std::memcpy(out_SR + c0 * n_periods, o.SR, (size_t)gc * np * 8);
            if (out_power_raw) std::memcpy(out_power_raw + c0 * n_periods, o.praw, (size_t)gc * np * 8);
        }
        // (pipelined: a group's time is the interval between two groups' results)
        const auto now = std::chrono::steady_clock::now();
        ctx->batch_group_ms[(size_t)g] = std::chrono::duration<double, std::milli>(now - last_done).count();
        last_done = now;
        return TLS_OK;
    };
    rc = enqueue_group(0);
    for (int64_t g = 0; g < n_groups && rc == TLS_OK; ++g) {
        if (g + 1 < n_groups && (rc = enqueue_group(g + 1))) break;
        rc = consume_group(g);
    }
    ctx->executed = false;   // the search ran on the batch slot, see search_batch_impl
    return rc;
}

int tls_grid_cells(const double* t, int64_t n, const double* periods, int64_t n_periods, const tls_template* tmpl,
                   const tls_params* params, int64_t* cells_per_period) {
    if (!t || !periods || !cells_per_period || n < 3 || n_periods < 0) {
        g_create_error = "tls_grid_cells: invalid argument";
        return TLS_E_ARG;
    }
    std::vector<tlsdev::WidthEntry> widths;
    int rc = build_widths(nullptr, tmpl, params, n, widths, nullptr);
    if (rc) return rc;
    double t_min, t_max;
    time_range(t, n, t_min, t_max);
    GridPlan gp;
    if (!plan_periods(widths, params, periods, n_periods, t_max - t_min, n, n + padded_width(widths), nullptr, cells_per_period, &gp)) {
        g_create_error = "tls_grid_cells: periods must be positive and finite";
        return TLS_E_ARG;
    }
    return TLS_OK;
}

int tls_debug_candidate_slabs(const int64_t* curve, int64_t n_fits, int64_t max_curves, int64_t max_fits, int64_t* out_slab,
                              int64_t* out_slot, int64_t* out_runs, int64_t* n_slabs) {
    if (n_fits < 0 || max_curves < 1 || max_fits < 1 || !n_slabs || (n_fits > 0 && (!out_slab || !out_slot || !out_runs))) {
        g_create_error = "tls_debug_candidate_slabs: invalid argument";
        return TLS_E_ARG;
    }
    std::vector<int> slot((size_t)std::min(max_fits, n_fits));
    tlsslab::Slab slab;
    *n_slabs = 0;
    for (int64_t f0 = 0; f0 < n_fits; f0 += (int64_t)slab.fits, ++*n_slabs) {
        tlsslab::next_slab(curve, n_fits, f0, (size_t)max_curves, (size_t)max_fits, slot.data(), slab);
        for (size_t i = 0; i < slab.fits; ++i) { out_slab[f0 + (int64_t)i] = *n_slabs; out_slot[f0 + (int64_t)i] = slot[i]; }
        out_runs[*n_slabs] = (int64_t)slab.runs.size();
    }
    return TLS_OK;
}

int tls_period_costs(const double* t, int64_t n, const double* periods, int64_t n_periods, const tls_template* tmpl,
                     const tls_params* params, double sigma, int64_t* cells_per_period, double* taps_per_period,
                     double* time_per_period, int64_t* workgroups_in_flight, const char* switches) {
    Switches po = process_options();
    if (!switches_parse(po, switches)) {
        g_create_error = "tls_period_costs: malformed switches (expected name=value,... of tls_debug_get_switches)";
        return TLS_E_ARG;
    }
    if (!t || !periods || !cells_per_period || !taps_per_period || n < 3 || n_periods < 0) {
        g_create_error = "tls_period_costs: invalid argument";
        return TLS_E_ARG;
    }
    std::vector<tlsdev::WidthEntry> widths;
    int rc = build_widths(nullptr, tmpl, params, n, widths, nullptr);
    if (rc) return rc;
    const int64_t M = n + padded_width(widths);
    double t_min, t_max;
    time_range(t, n, t_min, t_max);
    std::vector<tlsdev::PeriodRows> prow((size_t)n_periods);
    GridPlan gp;
    if (!plan_periods(widths, params, periods, n_periods, t_max - t_min, n, M, prow.data(), cells_per_period, &gp)) {
        g_create_error = "tls_period_costs: periods must be positive and finite";
        return TLS_E_ARG;
    }
    // expected template taps of a row: trial positions x taps x the fraction of windows of white noise whose mean
    // exceeds transit_depth_min (core.py:58): Q(depth_min * sqrt(d) / sigma)
    std::vector<double> prefix(widths.size() + 1, 0.0);
    for (size_t k = 0; k < widths.size(); ++k) {
        const auto& we = widths[k];
        const double n_pos = (double)((M - we.width) / we.xth + 1);
        double frac = 1.0;
        if (sigma > 0) frac = 0.5 * std::erfc(params->transit_depth_min * std::sqrt((double)we.width) / sigma / std::sqrt(2.0));
        prefix[k + 1] = prefix[k] + n_pos * (double)we.q_len * frac;
    }
    for (int64_t p = 0; p < n_periods; ++p)
        taps_per_period[p] = prefix[(size_t)prow[(size_t)p].k_hi] - prefix[(size_t)prow[(size_t)p].k_lo];
    if (time_per_period) {
        // Which kernel a search of this light curve runs: the plan and the pick tls_prepare and enqueue make, UNIFORM weights
        // assumed (the call has no dy: between the uniform and the per-point edges of the plan it prices a kernel a weighted
        // search does not run) and a normalised flux (it admits the fp32 screen: the choice between plain and screen is the
        // noise level's).  That kernel's measured cost per period in shader cycles: a0 + aN * n + b * cells + c * taps, fitted
        // to tls_debug_period_cycles on an MI355X (tools/gpu_cost_model.py, profiles/r03_cost_model_fit.json).  Only the
        // ratios matter to the callers (tls_amd/shard.py places block boundaries by the cumulative sum).
        SearchPlan plan;
        // (a series tls_prepare refuses is priced as the slab kernel it does not fit: the plan says `resident` either way)
        (void)plan_search(plan, n, widths, /*uniform=*/true, n_periods, visible_compute_units(), po);
        // kept from before the plan was shared: pruning is priced against the plain kernel's threshold
        // although the screen is assumed admissible, where a search takes the threshold beside the screen
        const bool prune_beside_screen = false;
        const FluxChoice flux = choose_flux_kernels(plan, po, widths, sigma, params->transit_depth_min,
                                                    screen_admissible(plan.resident, true, 0.0), prune_beside_screen);
        const Kernel kernel = pick_kernel(plan, flux);
        const bool resident = plan.resident, two_per_cu = plan.per_cu >= 2;
        double a0, aN, b, c;
        if (!resident) { a0 = 458384.0; aN = 4.5716; b = 0.4604; c = 0.03275; }        // HBM slab variant (TESS 27 d + Kepler 4 yr)
        else if (is_slim(kernel)) { a0 = 59538.0; aN = 0.0; b = 1.553; c = 0.2125; }    // LDS-resident, four 256-thread workgroups per CU (90 d at 50 ppm, round 5)
        else if (kernel == Kernel::ResidentPrune) { a0 = 116100.0; aN = 0.0; b = 1.906; c = 0.0125; }   // LDS-resident, pruning kernel (90 d at 500 ppm)
        else if (two_per_cu) { a0 = 54603.0; aN = 0.0; b = 0.7823; c = 0.1888; }        // LDS-resident, two 512-thread workgroups per CU (90 d)
        else { a0 = 56564.0; aN = 0.0; b = 0.3189; c = 0.1267; }                        // LDS-resident, one 1024-thread workgroup per CU (100 d)
        for (int64_t p = 0; p < n_periods; ++p)
            time_per_period[p] = a0 + aN * (double)n + b * (double)cells_per_period[p] + c * taps_per_period[p];
        // Series in the HBM slab: the coefficients are exact-mode measurements.  The search runs fast mode (enqueue; whatever
        // the number of periods or ranks: a period's mode depends on the light curve and the period alone): the plain prefix
        // sum saves ~3.5 cycles per point, a period pays an exact prefix pass (kBandHitCost of itself) with the probability that one of its
        // windows hits the undecided band, and a period that expects to hit it starts in exact mode (the same expectation as in
        // enqueue, for a normalised flux).  Without this the block of the longest periods came out a fifth late (PERF_LOG round 4).
        if (!resident && po.fast_slab != 0 && po.exact_prefix != 1 && sigma > 0) {
            const double eps = fast_mode_eps(M, 1.0 + 5.0 * sigma);
            const double band_max = po.band_max >= 0 ? po.band_max : kBandMax;
            std::vector<double> band;
            band_prefix_for(widths, sigma, params->transit_depth_min, eps, band, M);
            for (int64_t p = 0; p < n_periods; ++p) {
                const double lambda = band[(size_t)prow[(size_t)p].k_hi] - band[(size_t)prow[(size_t)p].k_lo];
                if (lambda > band_max) continue;                                  // starts in exact mode
                time_per_period[p] = (time_per_period[p] - 3.5 * (double)n) * (1.0 + kBandHitCost * std::min(1.0, lambda));
            }
        }
        // periods searched side by side on one GPU (one workgroup each): its CUs (256 on an MI355X; the first visible
        // device is asked, a process without one plans for an MI355X), two workgroups per CU when two folded series fit
        // its LDS.  A block of n periods takes ceil(n / this) rounds, not n / this.  (The cycle coefficients above are
        // MI355X measurements; only their ratios matter.)
        // (the classic kernel's registers let two of its workgroups be resident, however many its LDS share would admit)
        if (workgroups_in_flight) *workgroups_in_flight = (is_slim(kernel) ? plan.slim_slots : two_per_cu ? 2 : 1) * visible_compute_units();
    } else if (workgroups_in_flight) {
        *workgroups_in_flight = visible_compute_units();
    }
    return TLS_OK;
}

// ---- RCCL ---------------------------------------------------------------------------
int tls_comm_unique_id(char id_out[128]) {
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    ncclUniqueId id;
    ncclResult_t r = ncclGetUniqueId(&id);
    if (r != ncclSuccess) { g_create_error = std::string("ncclGetUniqueId: ") + ncclGetErrorString(r); return TLS_E_RCCL; }
    std::memcpy(id_out, &id, 128);
    return TLS_OK;
}

int tls_comm_init(tls_ctx* ctx, int n_ranks, int rank, const char id[128]) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (n_ranks < 1 || rank < 0 || rank >= n_ranks || !id) return fail(ctx, TLS_E_ARG, "bad rank layout");
    if (ctx->comm) return fail(ctx, TLS_E_STATE, "communicator already initialised");
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    ncclUniqueId uid;
    std::memcpy(&uid, id, 128);
    TLS_NCCL(ctx, ncclCommInitRank(&ctx->comm, n_ranks, uid, rank));
    ctx->n_ranks = n_ranks; ctx->rank = rank;
    TLS_HIP(ctx, ctx->d_scalar.reserve(2));
    return TLS_OK;
}

int tls_comm_destroy(tls_ctx* ctx) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (ctx->comm) { TLS_NCCL(ctx, ncclCommDestroy(ctx->comm)); ctx->comm = nullptr; }
    ctx->n_ranks = 1; ctx->rank = 0;
    return TLS_OK;
}

int tls_comm_info(tls_ctx* ctx, int* n_ranks, int* rank, int* device) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    int n = 0, r = -1, d = -1;
    if (ctx->comm) {
        TLS_NCCL(ctx, ncclCommCount(ctx->comm, &n));
        TLS_NCCL(ctx, ncclCommUserRank(ctx->comm, &r));
        TLS_NCCL(ctx, ncclCommCuDevice(ctx->comm, &d));
    }
    if (n_ranks) *n_ranks = n;
    if (rank) *rank = r;
    if (device) *device = d;
    return TLS_OK;
}

int tls_comm_allgather_device(tls_ctx* ctx, int64_t count_per_rank) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (!ctx->comm) return fail(ctx, TLS_E_STATE, "tls_comm_init first");
    if (!ctx->executed) return fail(ctx, TLS_E_STATE, "all-gather before tls_execute");
    if (count_per_rank < ctx->plan.n_periods || count_per_rank < 1) return fail(ctx, TLS_E_ARG, "count_per_rank smaller than this rank's shard");
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t c = (size_t)count_per_rank, np = (size_t)ctx->plan.n_periods, R = (size_t)ctx->n_ranks;
    // pack [chi2 | row | depth] of this shard, zero padded: 24 B per period
    TLS_HIP(ctx, ctx->d_pack.reserve(3 * c));
    TLS_HIP(ctx, ctx->d_gather.reserve(3 * c * R));
    TLS_HIP(ctx, hipMemsetAsync(ctx->d_pack.ptr, 0, 3 * c * 8, main_stream(ctx)));
    if (np) {
        TLS_HIP(ctx, hipMemcpyAsync(ctx->d_pack.ptr, ctx->d_chi2.ptr, np * 8, hipMemcpyDeviceToDevice, main_stream(ctx)));
        TLS_HIP(ctx, hipMemcpyAsync(ctx->d_pack.ptr + c, ctx->d_row.ptr, np * 8, hipMemcpyDeviceToDevice, main_stream(ctx)));
        TLS_HIP(ctx, hipMemcpyAsync(ctx->d_pack.ptr + 2 * c, ctx->d_depth.ptr, np * 8, hipMemcpyDeviceToDevice, main_stream(ctx)));
    }
    TLS_NCCL(ctx, ncclAllGather(ctx->d_pack.ptr, ctx->d_gather.ptr, 3 * c, ncclDouble, ctx->comm, main_stream(ctx)));
    ctx->gathered_count = (int64_t)c;
    return TLS_OK;
}

int tls_comm_fetch_gathered(tls_ctx* ctx, int64_t count_per_rank, double* all_chi2, int64_t* all_row, double* all_depth) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (!ctx->comm) return fail(ctx, TLS_E_STATE, "tls_comm_init first");
    if (!all_chi2 || !all_row || !all_depth) return fail(ctx, TLS_E_ARG, "null output");
    if (ctx->gathered_count != count_per_rank || count_per_rank < 1)
        return fail(ctx, TLS_E_STATE, "no device-side all-gather of that size to fetch");
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t c = (size_t)count_per_rank, R = (size_t)ctx->n_ranks;
    std::vector<double> host(3 * c * R);
    TLS_HIP(ctx, hipMemcpyAsync(host.data(), ctx->d_gather.ptr, host.size() * 8, hipMemcpyDeviceToHost, main_stream(ctx)));
    TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));
    for (size_t r = 0; r < R; ++r) {
        const double* blk = host.data() + r * 3 * c;
        std::memcpy(all_chi2 + r * c, blk, c * 8);
        std::memcpy(all_row + r * c, blk + c, c * 8);  // int64 bit patterns travel as 8-byte words
        std::memcpy(all_depth + r * c, blk + 2 * c, c * 8);
    }
    return TLS_OK;
}

int tls_comm_stage_results(tls_ctx* ctx, int64_t count_per_rank, int64_t slot, int64_t n_slots) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (!ctx->executed) return fail(ctx, TLS_E_STATE, "staging before tls_execute");
    if (count_per_rank < ctx->plan.n_periods || count_per_rank < 1 || n_slots < 1 || slot < 0 || slot >= n_slots)
        return fail(ctx, TLS_E_ARG, "bad slot layout");
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t c = (size_t)count_per_rank, np = (size_t)ctx->plan.n_periods;
    TLS_HIP(ctx, ctx->d_stage.reserve(3 * c * (size_t)n_slots));
    double* dst = ctx->d_stage.ptr + 3 * c * (size_t)slot;   // [chi2 | row | depth] of this slot, 24 B per period
    if (np < c) TLS_HIP(ctx, hipMemsetAsync(dst, 0, 3 * c * 8, main_stream(ctx)));
    if (np) {
        TLS_HIP(ctx, hipMemcpyAsync(dst, ctx->d_chi2.ptr, np * 8, hipMemcpyDeviceToDevice, main_stream(ctx)));
        TLS_HIP(ctx, hipMemcpyAsync(dst + c, ctx->d_row.ptr, np * 8, hipMemcpyDeviceToDevice, main_stream(ctx)));
        TLS_HIP(ctx, hipMemcpyAsync(dst + 2 * c, ctx->d_depth.ptr, np * 8, hipMemcpyDeviceToDevice, main_stream(ctx)));
    }
    return TLS_OK;
}

int tls_comm_allgather_staged(tls_ctx* ctx, int64_t count_per_rank, int64_t n_slots) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (!ctx->comm) return fail(ctx, TLS_E_STATE, "tls_comm_init first");
    if (count_per_rank < 1 || n_slots < 1) return fail(ctx, TLS_E_ARG, "bad slot layout");
    const size_t per_rank = 3 * (size_t)count_per_rank * (size_t)n_slots;
    if (ctx->d_stage.cap < per_rank) return fail(ctx, TLS_E_STATE, "nothing staged for that layout");
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    TLS_HIP(ctx, ctx->d_gather.reserve(per_rank * (size_t)ctx->n_ranks));
    TLS_NCCL(ctx, ncclAllGather(ctx->d_stage.ptr, ctx->d_gather.ptr, per_rank, ncclDouble, ctx->comm, main_stream(ctx)));
    ctx->gathered_count = -(int64_t)per_rank;   // marks a staged gather (tls_comm_fetch_gathered refuses it)
    return TLS_OK;
}

int tls_comm_fetch_staged(tls_ctx* ctx, int64_t count_per_rank, int64_t n_slots, int64_t slot, double* all_chi2,
                          int64_t* all_row, double* all_depth) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (!ctx->comm) return fail(ctx, TLS_E_STATE, "tls_comm_init first");
    if (!all_chi2 || !all_row || !all_depth) return fail(ctx, TLS_E_ARG, "null output");
    if (count_per_rank < 1 || n_slots < 1 || slot < 0 || slot >= n_slots) return fail(ctx, TLS_E_ARG, "bad slot layout");
    const size_t c = (size_t)count_per_rank, R = (size_t)ctx->n_ranks, per_rank = 3 * c * (size_t)n_slots;
    if (ctx->gathered_count != -(int64_t)per_rank) return fail(ctx, TLS_E_STATE, "no staged all-gather of that layout to fetch");
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<double> host(3 * c);
    for (size_t r = 0; r < R; ++r) {
        TLS_HIP(ctx, hipMemcpyAsync(host.data(), ctx->d_gather.ptr + r * per_rank + 3 * c * (size_t)slot, 3 * c * 8,
                                    hipMemcpyDeviceToHost, main_stream(ctx)));
        TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));
        std::memcpy(all_chi2 + r * c, host.data(), c * 8);
        std::memcpy(all_row + r * c, host.data() + c, c * 8);  // int64 bit patterns travel as 8-byte words
        std::memcpy(all_depth + r * c, host.data() + 2 * c, c * 8);
    }
    return TLS_OK;
}

int tls_comm_allgather_results(tls_ctx* ctx, int64_t count_per_rank, double* all_chi2, int64_t* all_row, double* all_depth) {
    int rc = tls_comm_allgather_device(ctx, count_per_rank);
    if (rc) return rc;
    return tls_comm_fetch_gathered(ctx, count_per_rank, all_chi2, all_row, all_depth);
}

int tls_comm_max(tls_ctx* ctx, double* value_inout) {
    if (!ctx) return fail(nullptr, TLS_E_ARG, "null context");
    if (!ctx->comm) return fail(ctx, TLS_E_STATE, "tls_comm_init first");
    TLS_HIP(ctx, hipSetDevice(ctx->device));
    TLS_HIP(ctx, hipMemcpyAsync(ctx->d_scalar.ptr, value_inout, 8, hipMemcpyHostToDevice, main_stream(ctx)));
    TLS_NCCL(ctx, ncclAllReduce(ctx->d_scalar.ptr, ctx->d_scalar.ptr + 1, 1, ncclDouble, ncclMax, ctx->comm, main_stream(ctx)));
    TLS_HIP(ctx, hipMemcpyAsync(value_inout, ctx->d_scalar.ptr + 1, 8, hipMemcpyDeviceToHost, main_stream(ctx)));
    TLS_HIP(ctx, hipStreamSynchronize(main_stream(ctx)));
    return TLS_OK;
}

int tls_comm_barrier(tls_ctx* ctx) {
    double v = 0;
    return tls_comm_max(ctx, &v);
}

}  // extern "C"
