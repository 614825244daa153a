// plan_sweep.hip -- the search planner (tls_amd/csrc/tls_plan.hip.h) over a sweep of inputs, host code only.
//
//   hipcc --offload-arch=gfx950 -O1 -std=c++17 -Xarch_host -fsanitize=address,undefined -o plan_sweep plan_sweep.hip && ./plan_sweep
//
// No device is touched.  Every plan is checked against what the kernels index by it (LDS sizes, tile bounds, the tile
// prefix, the live-unit lists), every pick against the plan; the sanitizers catch what the index arithmetic itself does
// wrong.  tests/test_plan_host.py builds and runs it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../tls_amd/csrc/tls_plan.hip.h"

using namespace tlsplan;

namespace {

long long g_checked = 0, g_refused = 0, g_slim = 0, g_slim512 = 0, g_slab = 0, g_oversize = 0, g_split = 0;

#define CHECK(cond)                                                                                              \
    do {                                                                                                         \
        if (!(cond)) {                                                                                           \
            std::fprintf(stderr, "plan_sweep: %s failed (line %d): n %lld uniform %d table %d periods %lld set %d\n", #cond, \
                         __LINE__, (long long)n, (int)uniform, table, (long long)n_periods, set);              \
            std::exit(1);                                                                                        \
        }                                                                                                        \
    } while (0)

// distinct widths int(duration * n) of a geometric duration grid up to `widest` of the series, at most `cap` of them;
// strides as build_widths forms them for T0_fit_margin = 0.01
std::vector<tlsdev::WidthEntry> width_table(int64_t n, double widest, double step, size_t cap) {
    std::vector<int> w;
    for (double d = 0.0005; d <= widest; d *= step) {
        const int wd = (int)(d * (double)n);
        if (wd >= 1 && (w.empty() || wd > w.back())) w.push_back(wd);
    }
    if (w.empty()) w.push_back(1);
    while (w.size() > cap) {   // thin evenly, keep the widest
        std::vector<int> kept;
        for (size_t k = 0; k < w.size(); ++k) if (k % 2 == (w.size() - 1) % 2) kept.push_back(w[k]);
        w.swap(kept);
    }
    std::vector<tlsdev::WidthEntry> out;
    for (int wd : w) {
        tlsdev::WidthEntry we;
        std::memset(&we, 0, sizeof we);
        we.width = wd; we.q_len = wd; we.row = (int)out.size();
        we.xth = std::max(1, (int)((double)wd / 100.0));
        we.tiled = tlsdev::row_is_tiled(we.width, we.xth) ? 1 : 0;
        we.prunable = 1; we.inv_d = 1.0 / wd;
        out.push_back(we);
    }
    return out;
}

Switches switch_set(int set) {
    Switches o;
    std::memset(&o, 0, sizeof o);
    o.exact_prefix = o.slim = o.prune = o.screen32 = o.no_screen = o.fast_slab = o.x_staged = o.split = o.split_batch = -1;
    o.sort2 = o.threads = o.blocks = o.plan_threads = o.t0_rot = o.reg_scan = -1;
    o.prune_min_live = -1; o.perm_table = -1; o.band_max = -1.0;
    switch (set) {
        case 1: o.slim = 0; break;
        case 2: o.exact_prefix = 1; break;
        case 3: o.prune = 1; break;
        case 4: o.screen32 = 1; break;
        case 5: o.threads = 512; break;
        case 6: o.fast_slab = 0; break;
        default: break;
    }
    return o;
}

void check_plan(int64_t n, bool uniform, int table, int64_t n_periods, int set) {
    std::vector<tlsdev::WidthEntry> widths = table == 0   ? width_table(n, 0.12, 1.1, 1000)
                                             : table == 1 ? width_table(n, 0.36, 1.1, 1000)
                                                          : width_table(n, 0.12, 1.004, 110);
    const size_t nw = widths.size();
    std::vector<tlsdev::PeriodRows> prow((size_t)n_periods);
    std::vector<int> order((size_t)n_periods);
    for (int64_t p = 0; p < n_periods; ++p) {
        tlsdev::PeriodRows& pr = prow[(size_t)p];
        pr.k_lo = (int)((p * 3) % (int64_t)(nw / 2 + 1));
        pr.k_hi = p % 17 == 16 ? pr.k_lo : pr.k_lo + 1 + (int)((p * 7) % (int64_t)(nw - (size_t)pr.k_lo));   // (a period in 17 without a row)
        pr.k_x = pr.k_lo; pr.pad = 0;
        order[(size_t)p] = (int)(n_periods - 1 - p);
    }
    const Switches opt = switch_set(set);
    const int n_cu = 256;
    SearchPlan plan;
    const char* why = plan_search(plan, n, widths, uniform, n_periods, n_cu, opt, prow.data(), order.data());
    ++g_checked;
    if (why) { CHECK(!plan.resident); ++g_refused; return; }
    const int64_t M = plan.M;
    g_slim += plan.slim_blocks > 0 && plan.slim_threads == tlsdev::kSlimThreads; g_slim512 += plan.slim_blocks > 0 && plan.slim_threads == tlsdev::kSlimThreadsWide;
    g_slab += !plan.resident; g_oversize += plan.any_oversize; g_split += plan.split;
    CHECK(plan.n == n && plan.M == n + plan.W && plan.W % 2 == 0 && plan.W >= widths.back().width && plan.n_widths == (int)nw);
    CHECK(plan.lds_bytes <= kLdsPerCU && plan.lds_bytes >= (size_t)plan.hdr_bytes);
    CHECK((size_t)plan.hdr_bytes == lds_header_bytes(nw));
    CHECK(plan.blocks >= 1 && plan.threads >= 64 && plan.threads <= 1024 && plan.threads % 64 == 0);
    CHECK(plan.nb >= 1 && plan.nb <= n && (size_t)plan.hdr_bytes + 4 * (size_t)plan.nb <= kLdsPerCU);
    if (plan.slim_blocks > 0) {
        CHECK(plan.resident && uniform && plan.slim_slots >= 2 && plan.slim_slots <= 4);
        CHECK(plan.slim_lds * (size_t)plan.slim_slots <= kLdsPerCU);
        CHECK(plan.slim_blocks <= plan.slim_slots * n_cu);
        CHECK(n <= (int64_t)plan.slim_threads * tlsdev::kSlimPer);
        CHECK(plan.perm_table_want == 0 || plan.perm_table_want == (size_t)n_periods * (size_t)tlsdev::slim_perm_row(plan.slim_threads));
    } else {
        CHECK(plan.slim_slots == 0 && plan.slim_lds == 0 && plan.perm_table_want == 0 && plan.slim_perm_per == 0);
    }
    if (plan.resident) {
        CHECK(n <= 65535 && plan.tile_len == 0 && plan.tile_halo == 0 && !plan.split && !plan.any_oversize && plan.per_cu >= 1);
        CHECK((size_t)plan.per_cu * plan.lds_bytes <= kLdsPerCU);
        CHECK(plan.lds_bytes == (size_t)plan.hdr_bytes + (uniform ? 2 : 3) * 8 * (size_t)(M + 1 + plan.region_pad));
    } else {
        const size_t buffers = uniform ? 1 : 2;
        CHECK(plan.tile_len > 0 && plan.tile_len % 320 == 0 && plan.tile_halo > 0);
        CHECK((size_t)plan.hdr_bytes + buffers * 8 * ((size_t)plan.tile_len + (size_t)plan.tile_halo) <= plan.lds_bytes);
        CHECK((size_t)plan.hdr_bytes + 8 * ((size_t)plan.cumsum_round + 4) <= plan.lds_bytes);
        CHECK(plan.blocks <= n_cu && plan.split_blocks >= 1 && plan.split_batch >= 1 && plan.scratch_doubles > 0);
        bool any = false;
        for (const auto& we : widths) {
            any = any || we.oversize;
            CHECK(!we.oversize || (!we.tiled && !we.prunable));
            CHECK(we.oversize || (size_t)we.width < (size_t)plan.tile_halo);
        }
        CHECK(any == plan.any_oversize);
        CHECK(!plan.split_fast || (uniform && !any && n % 2 == 0));
        uint64_t tiles = 0;
        for (int64_t p = 0; p < n_periods; ++p) {
            const int pad = prow[(size_t)p].pad;
            CHECK(pad == 0 || (pad > plan.tile_len && pad % 320 == 0 && pad < plan.tile_len + plan.tile_halo));
            const int64_t tl = pad > 0 ? pad : plan.tile_len;
            tiles += (uint64_t)((M + tl - 1) / tl);
        }
        if (plan.split) {
            CHECK(plan.tile_prefix.size() == (size_t)n_periods + 1 && plan.tile_prefix[0] == 0);
            for (int64_t p = 0; p < n_periods; ++p) CHECK(plan.tile_prefix[(size_t)p + 1] > plan.tile_prefix[(size_t)p]);
            CHECK(plan.tile_prefix[(size_t)n_periods] == tiles);
            CHECK(plan.split_max_items >= 1 && plan.split_max_items <= (int64_t)tiles);
        }
    }
    size_t chunks = 0;
    for (const auto& we : widths) {
        CHECK(we.list_base == (int)chunks && we.n_pos >= 1 && we.n_chunks >= 1 && we.n_chunks <= we.n_pos);
        CHECK((int64_t)(we.n_pos - 1) * we.xth + we.width <= M);
        chunks += (size_t)we.n_chunks;
    }
    CHECK(plan.list_stride >= chunks && plan.list_stride % 64 == 0);
    CHECK(plan.p2_shift >= 4 && (((size_t)M + ((size_t)1 << plan.p2_shift) - 1) >> plan.p2_shift) <= (size_t)tlsdev::kP2MaxBlocks);
    // every pick: the flux's eight choices, a plain / counting / debug launch, one curve and a batch
    for (int f = 0; f < 8; ++f)
        for (int l = 0; l < 8; ++l) {
            FluxChoice flux;
            flux.admissible = (f & 1) != 0 && plan.resident && uniform;   // (screen_admissible)
            flux.prune = (f & 2) != 0; flux.screen = (f & 4) != 0;
            LaunchFlags launch;
            launch.count_work = (l & 1) != 0; launch.debug_entry = (l & 2) != 0; launch.batch_curves = (l & 4) ? 32 : 1;
            const Kernel k = pick_kernel(plan, flux, launch);
            CHECK(!is_slim(k) || (plan.slim_blocks > 0 && !launch.debug_entry));
            CHECK((k == Kernel::Slim512) == (is_slim(k) && plan.slim_threads == tlsdev::kSlimThreadsWide));
            CHECK((k == Kernel::Slab || k == Kernel::SlabSplit) == !plan.resident);
            CHECK(k != Kernel::SlabSplit || (plan.split && launch.batch_curves == 1));
            CHECK((k != Kernel::ResidentPrune && k != Kernel::ResidentScreen) || (plan.resident && uniform && !launch.count_work));
            CHECK(kernel_name(k)[0] != 0);
        }
}

}  // namespace

int main() {
    std::vector<int64_t> lengths;
    for (double x = 100; x < 200000; x *= 1.06) lengths.push_back((int64_t)x | 1), lengths.push_back(((int64_t)x | 1) + 1);
    for (int64_t n = 2000; n < 9600; n += 61) lengths.push_back(n);              // the shares of the LDS, resident to slab
    for (int64_t n = 5100; n <= 5140; ++n) lengths.push_back(n);                 // 256 threads x 20 points
    for (int64_t n = 10220; n <= 10260; ++n) lengths.push_back(n);               // 512 threads x 20 points
    for (int64_t n = 65520; n <= 65550; ++n) lengths.push_back(n);               // 16-bit orders
    lengths.push_back(200000);
    const int64_t period_counts[] = {1, 60, 300, 5000};
    for (int64_t n : lengths)
        for (int uniform = 0; uniform < 2; ++uniform)
            for (int table = 0; table < 3; ++table)
                for (int64_t n_periods : period_counts)
                    for (int set = 0; set < 7; ++set) check_plan(n, uniform != 0, table, n_periods, set);
    std::printf("%lld plans checked, %lld refused; four-slot %lld, its 512-thread shape %lld, slab %lld (oversize rows %lld, two roles %lld)\n",
                g_checked, g_refused, g_slim, g_slim512, g_slab, g_oversize, g_split);
    // (a sweep that met no plan of a family checked nothing about it)
    return g_slim && g_slim512 && g_slab && g_oversize && g_split ? 0 : 2;
}
