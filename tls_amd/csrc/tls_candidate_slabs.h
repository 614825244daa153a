// tls_candidate_slabs.h -- host only, no HIP: how a per-candidate survey stage cuts its candidates into slabs
// (DESIGN.md "Candidate slabs").  A slab is a run of consecutive candidates that fits the stage's device buffers: at most
// max_fits candidates reading at most max_curves distinct light curves, each curve copied once into a slot of the slab.
#pragma once

#include <cstddef>
#include <cstdint>
#include <unordered_map>
#include <vector>

namespace tlsslab {

struct Run { int64_t curve; size_t slot, count; };      // consecutive curves in consecutive slots: one copy

struct Slab {
    size_t fits = 0;        // candidates f0 .. f0 + fits - 1
    size_t curves = 0;      // slots used
    std::vector<Run> runs;  // the curves of slots 0 .. curves - 1, coalesced
    std::unordered_map<int64_t, int> slot_of;   // (working state, kept for its buckets)
};

// The slab that starts at candidate f0 < n_fits (max_curves, max_fits >= 1); slot[i] receives the slot of candidate f0 + i.
// Candidate f reads curve[f], or curve f where curve is null.  Slots are handed out in order of first appearance; a candidate
// whose curve is new when every slot is taken starts the next slab (a slab's first candidate always finds a slot); a run
// grows only by the curve that follows its last one, which then also lies in the next slot.
inline void next_slab(const int64_t* curve, int64_t n_fits, int64_t f0, size_t max_curves, size_t max_fits, int* slot, Slab& s) {
    s.slot_of.clear();
    s.runs.clear();
    s.fits = 0;
    while (f0 + (int64_t)s.fits < n_fits && s.fits < max_fits) {
        const int64_t f = f0 + (int64_t)s.fits, c = curve ? curve[f] : f;
        auto it = s.slot_of.find(c);
        if (it == s.slot_of.end()) {
            if (s.slot_of.size() == max_curves) break;
            const size_t next = s.slot_of.size();
            it = s.slot_of.emplace(c, (int)next).first;
            if (!s.runs.empty() && s.runs.back().curve + (int64_t)s.runs.back().count == c) ++s.runs.back().count;
            else s.runs.push_back(Run{c, next, 1});
        }
        slot[s.fits++] = it->second;
    }
    s.curves = s.slot_of.size();
}

}  // namespace tlsslab
