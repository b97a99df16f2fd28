// leaflet_rows.h — which row of the flag block every frame of a batch is routed by, for the methods that assign on the device
// (host part of leaflets.rs:435-441, 1437-1472).  Row 0 is the assignment carried over from earlier batches
// (AssignedLeaflets::local, leaflets.rs:1371-1380), rows 1.. are the assignment frames of this batch in order.  No HIP call
// and no handle in here, so tests/cabi/leaflet_rows.cpp can drive all of it without a device.  (The whole-trajectory manual
// table plans its rows in replay_rows.h.)
#ifndef GORDER_LEAFLET_ROWS_H
#define GORDER_LEAFLET_ROWS_H

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/gorder_hip.h"
#include "replay_rows.h"

namespace gorder {

// NoClusters: spectral clustering, the batch's first assignment frame is not frame 0 and the handle holds no clusters of an
// earlier one to match against.  NotPrimed: a frame comes before every assignment, in this batch and before it.
enum LeafletRowsStatus { kLeafletRowsOk = 0, kLeafletRowsNoClusters = 1, kLeafletRowsNotPrimed = 2 };

// arow[f]: the row frame f reads; aframes: the frames (positions in the batch) that assign = rows 1..; last_assign_frame: the
// trajectory frame of the newest assignment, left as it is when the batch has none.  Spectral clustering only: `is0` is
// emptied at the first assignment frame and then holds, per assignment frame, whether it is frame 0 of the trajectory (it is
// not touched when the batch assigns nothing, and is left empty by NoClusters).  Anything but Ok: the rows are not to be used.
inline LeafletRowsStatus plan_assignment_rows(uint32_t method, uint32_t frequency, bool have_assignment, bool cl_have_carry,
                                              const uint64_t *frame_index, uint32_t n_frames, std::vector<uint32_t> &arow,
                                              std::vector<uint32_t> &aframes, std::vector<uint8_t> &is0,
                                              uint64_t &last_assign_frame) {
    arow.assign(n_frames, 0u);
    aframes.clear();
    uint32_t cur = 0;
    bool have = have_assignment;
    for (uint32_t f = 0; f < n_frames; f++) {
        if (method != GORDER_LEAFLETS_MANUAL && replay_should_assign(frequency, frame_index[f])) {
            if (method == GORDER_LEAFLETS_CLUSTERING) {
                // a later assignment frame is matched against the clusters the handle holds
                if (aframes.empty()) is0.clear();
                if (aframes.empty() && frame_index[f] != 0 && !cl_have_carry) return kLeafletRowsNoClusters;
                is0.push_back(frame_index[f] == 0 ? 1 : 0);
            }
            aframes.push_back(f);
            cur = (uint32_t)aframes.size();
            have = true;
            last_assign_frame = frame_index[f];
        }
        if (!have) return kLeafletRowsNotPrimed;
        arow[f] = cur;
    }
    return kLeafletRowsOk;
}

}  // namespace gorder

#endif
