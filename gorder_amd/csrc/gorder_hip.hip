// gorder_hip.hip — MI355X (gfx950) lipid-order engine: host side + C ABI; the kernels live in kernels_*.h.
//
// Path accelerated (reference file:line under /root/reference/src/analysis):
//   analyze_frame                      common.rs:201-235
//   MoleculeTypes::analyze_frame       topology/molecule.rs:54-95
//   BondType::analyze_frame            topology/bond.rs:396-446      -> k_bonds_tiled / k_bonds_direct
//   BondLike::add_order                topology/bond.rs:184-215         (register accumulators)
//   calc_sch / vector_to               mod.rs:78-82, pbc.rs:378-385     (gm_math.h)
//   OrderValue / AnalysisOrder         order.rs:13-66, 178-188          (i64 ticks, u64 counts)
//   check_box                          common.rs:186-198             -> k_batch_end (k_check_box for a priming frame)
//   SystemLeafletClassification::run   leaflets.rs:171-205           -> k_leaflets_global
//   common_identify_leaflet            leaflets.rs:711-732              (same kernel)
//   IndividualClassification           leaflets.rs:777-801           -> k_leaflets_individual
//   SystemSphericalClusterClassification spherical_clustering.rs:42-277, leaflets.rs:1296-1366 -> k_leaflets_spherical
//   SystemClusterClassification (precise route) clustering.rs:478-800 -> k_cluster_{degrees,lanczos,embed,orient}
//   LocalClassification + local centres leaflets.rs:661-675, pbc.rs:273-318 -> k_local_{build,rowprefix,decide,flags_rows,flags_todo} (k_local_{bin,scan,scatter,flags}: very large membranes, no box)
//   should_assign / get_assigned       leaflets.rs:435-441, 1437-1472   (host: leaflet_rows.h)
//   SystemTopology::add / reduce       topology/mod.rs:236-272          (integer sums: order-free)
//
// Built for gfx950 only.  No CPU fallback: without a device every entry point fails loudly.
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <deque>
#include <type_traits>
#include <vector>

#include "../../include/gorder_hip.h"
#include "gm_math.h"
#include "plan.h"
#include "collect_store.h"
#include "device_mem.h"
#include "replay_rows.h"
#include "leaflet_rows.h"
#include "timewise_blocks.h"
#include "ordermap_final.h"
#include "order_route.h"
#include "molecule_rows.h"
#include "ua_molecule_rows.h"
#include "order_hist.h"
#include "bond_corr.h"
#include "neighbour_classes.h"
#include "switches.h"

#pragma clang fp contract(off)

using gorder::DirectItem;
using gorder::Item;
using gorder::kBlock;
using gorder::Plan;
using gorder::Tile;

#include "kernels_common.h"
#include "kernels_tile.h"
#include "kernels_bonds.h"
#include "kernels_extras.h"
#include "kernels_ua.h"
#include "kernels_molrows.h"
#include "kernels_radial.h"
#include "kernels_neighbours.h"
#include "kernels_hist.h"
#include "kernels_ua_samples.h"
#include "kernels_corr.h"
#include "kernels_leaflets.h"
#include "kernels_cluster.h"
#include "kernels_cluster_cutoff.h"
#include "kernels_normals.h"
#include "kernels_xtc.h"
#include "kernels_trr.h"
#include "kernels_collect.h"
#include "kernels_replay.h"
#include "kernels_timewise.h"
#include "kernels_ordermap.h"

// ============================================================================================
// host side
// ============================================================================================

// ---- who owns what (device_mem.h): device and pinned blocks, events and streams that free themselves ----------------------
struct DeviceMem {
    static void *alloc(size_t bytes) { void *p = nullptr; return hipMalloc(&p, bytes) == hipSuccess ? p : nullptr; }
    static void release(void *p) { (void)hipFree(p); }
};
struct PinnedMem {
    static void *alloc(size_t bytes) { void *p = nullptr; return hipHostMalloc(&p, bytes) == hipSuccess ? p : nullptr; }
    static void release(void *p) { (void)hipHostFree(p); }
};
template <typename T> using DBuf = gorder::Buf<T, DeviceMem>;
template <typename T> using HBuf = gorder::Buf<T, PinnedMem>;
using u64 = unsigned long long;

struct Event {
    hipEvent_t ev = nullptr;
    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    ~Event() { if (ev) (void)hipEventDestroy(ev); }
    hipError_t create(unsigned flags = hipEventDisableTiming) { return ev ? hipSuccess : hipEventCreateWithFlags(&ev, flags); }
    operator hipEvent_t() const { return ev; }
};
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    hipError_t create() { return s ? hipSuccess : hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
    operator hipStream_t() const { return s; }
};

// an accumulator block of `words` u64 and the replicas the kernels add into (k_fold_replicas folds them): radial shells, order
// distributions
struct RepAcc {
    DBuf<u64> acc, rep;      // [words], [n_rep][words]
    uint32_t n_rep = 1;
    size_t words = 0;
    bool alloc(size_t n_words, uint32_t n_rep_wanted) {
        words = n_words;
        n_rep = gorder::replica_count(n_rep_wanted, n_words);
        return acc.alloc(words) && rep.alloc((size_t)n_rep * words);
    }
    void reset() { acc.reset(); rep.reset(); words = 0; }
    hipError_t zero_async(hipStream_t stream) {
        const hipError_t e = hipMemsetAsync(acc, 0, words * sizeof(u64), stream);
        return e != hipSuccess ? e : hipMemsetAsync(rep, 0, (size_t)n_rep * words * sizeof(u64), stream);
    }
    hipError_t fold(hipStream_t stream) {
        hipLaunchKernelGGL(k_fold_replicas, dim3((uint32_t)((words + 255) / 256)), dim3(256), 0, stream, acc.get(), rep.get(), n_rep, (uint32_t)words);
        return hipGetLastError();
    }
};

// bond reorientation (gorder_hip_set_bond_correlation; bond_corr.h, kernels_corr.h): the lags, the ring of frame planes
// float4 [ring_planes][plane_items] (allocated at the first submit), the sums and counts [n_lags][4][n_acc] laid out like d_acc
// per lag and their replicas (k_bond_corr adds into them)
struct BondCorr {
    std::vector<uint32_t> lags;                 // empty: off
    DBuf<uint32_t> d_lags;                      // padded to whole groups of kCorrLagBlock with kCorrNoLag
    DBuf<float4> ring;
    uint32_t ring_planes = 0, subrange = 0;     // R = max lag + subrange; 0: no ring yet
    uint32_t plane_items = 0;                   // n_tiles * kBlock
    uint64_t seen = 0;                          // analysed frames since create / reset: frame g lives in plane g mod R
    RepAcc acc;
    bool on() const { return !lags.empty(); }
};

// order by local composition (gorder_hip_set_neighbour_classes; neighbour_classes.h, kernels_neighbours.h): the centre atom of
// every molecule and the neighbour atoms on the device and on the host (the payload of an undefined position), the class bytes
// [frames][n_mol_total] of the last batch (k_neighbour_counts writes them, k_bonds_classes reads them), the sums and counts
// [n_classes][4][n_acc] laid out like d_acc per class and their replicas (k_bonds_classes adds into them)
struct NeighbourClasses {
    uint32_t n_classes = 0;                     // 0: off
    float radius = 0.0f, thr = 0.0f;            // thr = local_radius_threshold(radius)
    std::vector<uint32_t> centres, neighbours;
    DBuf<uint32_t> d_centres, d_neighbours;
    DBuf<uint8_t> rows;
    uint32_t rows_frames = 0;                   // frames the rows hold right now (the last batch, or its last sub-range)
    RepAcc acc;
    size_t lds_bytes = 0;                       // the LDS table of the widest tile
    bool direct = false;                        // per-sample global atomics: the table does not fit, or GORDER_HIP_NB_DIRECT
    bool on() const { return n_classes != 0; }
};

struct gorder_hip_handle {
    gorder::Switches sw;                // the GORDER_HIP_* switches as gorder_hip_create found them; nothing writes them afterwards
    // staging buffers of gorder_hip_run_trajectory, kept between calls (trajectory_driver.h: TrajCache)
    void *traj_cache = nullptr;
    void (*traj_cache_free)(gorder_hip_handle *) = nullptr;
    Plan plan;
    gorder_tables_t tables{};           // scalar copy (pointers inside are NOT kept)
    int device = 0;
    Stream own_stream;                  // (declared before every buffer: destroyed after them)
    hipStream_t stream = nullptr;
    // device tables
    DBuf<Tile> d_tiles;
    DBuf<Item> d_items;
    DBuf<uint32_t> d_tile_slots;
    DBuf<DirectItem> d_direct;
    DBuf<Tile> d_ua_tiles;
    DBuf<gorder::UaItem> d_ua_items;
    DBuf<uint32_t> d_ua_tile_slots;
    // ordermaps [3][n_acc][nx*ny] and timewise rows [cap][3][n_acc]
    uint32_t map_nx = 0, map_ny = 0;
    DBuf<u64> d_map_sums, d_map_cnts;   // [3][n_acc][nx*ny], folded
    DBuf<u64> d_map_packed;             // [1 or 2][n_acc][nx*ny], what the kernels add into
    DBuf<u64> d_map_rec;                // united-atom staging for k_map_accumulate (see ExtraArgs::map_rec)
    DBuf<gorder::MapRun> d_ua_runs, d_runs;
    DBuf<uint32_t> d_ua_run_begin, d_run_begin;
    DBuf<Item> d_items_by_slot;
    DBuf<uint32_t> d_ua_item_run, d_item_run;
    DBuf<uint4> d_lgrid;            // per slab frame: the cell grid of the local-leaflet kernels
    DBuf<LocalRowPre> d_lrowpre;    // per slab frame: prefix sums along the rows of cells (k_local_rowprefix)
    DBuf<LocalEdge> d_ledge;        // the same cells' 16-byte entries for the bound of k_local_flags_rows
    DBuf<float4> d_lfinfo;          // per slab frame: extrema of the membrane's normal coordinate, finite flag
    // k_local_decide pays when it decides whole frames; a membrane whose heads it leaves open (one that undulates by more than
    // the water around it allows) is better off without it: every submit that runs it reports {frames left open, frames}
    // to pinned memory, and a submit that finds the majority open sends the next kDecidePause submits down the rows kernel
    // alone.  (Either way the sides are the reference's: the choice is about time only.)
    static constexpr uint32_t kDecidePause = 16;
    DBuf<uint32_t> d_lsummary;
    HBuf<uint32_t> h_lsummary;
    Event lsummary_written;
    bool lsummary_pending = false;
    uint32_t decide_pause = 0;
    uint64_t decide_submits = 0, decide_paused_submits = 0;
    DBuf<uint32_t> d_lneed;         // [local_slab + 1] heads of each slab frame k_local_decide left to k_local_flags_rows; any of the slab
    DBuf<uint2> d_ltodo;            // {count}, then the (slab frame, head) pairs left to the general passes
    size_t map_lds_bytes = 0;
    bool map_staged = false;       // the packed map of one slot fits LDS: stage + accumulate instead of one atomic per sample
    uint64_t map_pending = 0;      // upper bound of the samples one packed word may hold since the last fold
    uint32_t map_max_mol = 1;      // most molecules of one type = most samples per tile and frame
    DBuf<u64> d_tw_sums, d_tw_cnts;
    uint64_t tw_cap = 0;               // rows (frames) those two hold
    // scratch of the passes over those rows (kernels_timewise.h): block sums then counts [2][n_blocks][3][n_acc], the groups in
    // CSR form, the groups' per-frame rows and their chunk totals [2][..][3][n_groups], carry and end [4][3][n_groups], the columns
    DBuf<u64> d_twx_blocks, d_twx_rows, d_twx_totals, d_twx_edge;
    DBuf<uint32_t> d_twx_groups;
    DBuf<float> d_twx_out;
    // scratch of gorder_hip_ordermaps (kernels_ordermap.h): the groups in CSR form, the finished maps [n_groups][3][nx*ny]
    DBuf<uint32_t> d_omx_groups;
    DBuf<float> d_omx_out;
    ExtraArgs extra{};
    DBuf<uint32_t> d_geom_group;
    DBuf<float> d_shapes;
    DBuf<float> d_inv_box;             // GORDER_FLAG_UA_FAST_NORMALISE: 1 / box edge per frame of the batch
    // dynamic membrane normals: cloud + per-molecule heads, cell-list scratch (dyn_slab frames), normals of the batch
    uint32_t dyn_slab = 4, local_slab = 4;
    bool local_halo = false;           // local leaflets: rows of cells with a halo + prefix sums (k_local_flags_rows)
    size_t local_rec_stride = 0;       // records per slab frame the local-leaflet record arrays hold
    DBuf<XtcCheckpoint> d_xtc_cp;      // gorder_hip_xtc_decode: where the chunks of the frames start (k_xtc_scan -> k_xtc_chunks)
    bool dyn = false;
    DBuf<uint32_t> d_dyn_cloud, d_dyn_heads;
    DBuf<uint32_t> d_dyn_cell_of, d_dyn_count;
    DBuf<float> d_dyn_rec;
    DBuf<float4> d_dyn_normals;
    DBuf<DynCov> d_dyn_cov;            // per (slab frame, molecule): the sums of k_dyn_cov for k_dyn_eigen
    std::vector<float> last_normals;   // [n_mol_total][4] of the last submitted frame
    // manual membrane normals (ManualMembraneNormal, normal.rs:266-300): handed over per batch by the host
    std::vector<float> manual_normals; // [frames][n_mol_total][4] (nx, ny, nz, 3) for the NEXT submit
    uint32_t manual_frames = 0;
    bool manual_active = false;        // this batch's samples read d_dyn_normals filled from manual_normals
    DBuf<uint32_t> d_err;
    u64 *d_acc = nullptr;              // [4][n_acc] + total_frames: a view of own_acc, or of the memory gorder_hip_bind_accumulators bound
    DBuf<u64> own_acc;                 // the block the handle allocated itself (empty once external memory is bound)
    DBuf<u64> d_rep;                   // [sw.replicas][4][n_acc] (see k_fold_replicas; GORDER_HIP_REPLICAS)
    bool rep_dirty = false;
    size_t acc_words = 0;
    // leaflets
    DBuf<uint32_t> d_heads, d_membrane, d_methyl_begin, d_methyl_atoms;
    DBuf<uint8_t> d_aflags;
    size_t aflags_rows = 0;            // rows of n_mol_total flags it holds
    DBuf<float> d_adist;
    // spherical clustering: distances of the group atoms past the register-resident ones, sph_slab assignment frames a launch;
    // the statistics of the most recent assignment frame (gorder_hip_spherical_stats)
    DBuf<float> d_sph_spill, d_sph_stats;
    uint32_t sph_spill = 0, sph_slab = 1u << 20, sph_threads = 1024;
    // spectral clustering: scratch for cl_slab assignment frames a launch (one allocation, carved in ClArgs), the group slot
    // of every molecule's head, the oriented labels of the previous assignment frame (the carry) and the last frame's statistics
    DBuf<char> d_cl_scratch;
    DBuf<uint32_t> d_cl_head_slot;
    DBuf<uint8_t> d_cl_carry, d_cl_is0;
    DBuf<float> d_cl_stats;
    uint32_t cl_slab = 1, cl_m_max = 0;
    bool cl_have_carry = false;
    bool cl_cut = false;                   // GORDER_FLAG_CLUSTER_CUTOFF: kernels_cluster_cutoff.h, its own scratch layout
    uint32_t cl_tiles = 0, cl_sort = 0;    // row tiles and counting-sort blocks of a frame (cut-off route)
    std::vector<uint8_t> cl_is0;           // per assignment frame of the call in flight: frame_index == 0
    // Local leaflets scratch (sized for local_slab assignment frames)
    DBuf<uint32_t> d_lcell_of, d_lcell_count, d_lcell_fill;
    DBuf<float> d_ltrig;               // LocalRec records, as LocalArgs::trig takes them
    DBuf<uint32_t> d_arow, d_aframes;
    // what those two hold right now: equal batches (same length, same assignment pattern) skip the upload
    std::vector<uint32_t> up_arow, up_aframes;
    bool up_arow_valid = false, up_aframes_valid = false;      // (a new allocation holds nothing yet)
    bool have_assignment = false;
    uint64_t assignment_frame = 0;
    // one read for global leaflets + order parameters (Plan::spec_ok; k_bonds_tiled<..., MOM> + k_spec_*)
    bool spec_enabled = false;         // the plan allows it and GORDER_HIP_NO_SPECULATE is not set
    DBuf<uint2> d_own;
    DBuf<float4> d_mom;
    DBuf<float> d_head_z;
    DBuf<uint32_t> d_own_head_begin;
    DBuf<uint2> d_own_heads;
    DBuf<float> d_spec_center;
    DBuf<uint8_t> d_spec_ok;
    DBuf<uint32_t> d_spec_counters;                // two pairs (batches alternate): [0] mispredicted (frame, molecule) pairs, [1] frames left to the exact kernel
    // pinned copies of the last speculative batches' counters, looked at (without waiting) when a later batch is submitted
    static constexpr uint32_t kSpecRing = 8;
    HBuf<uint32_t> h_spec_counters;                // [kSpecRing][2]
    Event spec_counters_copied[kSpecRing];
    uint64_t spec_ring_frames[kSpecRing] = {};     // frames of the batch in that slot (0: nothing pending)
    DBuf<uint32_t> d_spec_mol_begin;
    DBuf<SpecSample> d_spec_samples;
    uint64_t spec_batches = 0, spec_fixed = 0, spec_exact_frames = 0;   // statistics (gorder_hip_speculation_stats)
    // host staging for submit_host: two device buffers, filled on a copy stream while the kernels of the other one run
    DBuf<float> d_stage_xyz[2], d_stage_box[2];
    Event stage_copied[2], stage_computed[2];
    bool stage_used[2] = {false, false};
    int stage_next = 0;
    Stream copy_stream;
    float n2 = 1.0f, n2sq = 1.0f;
    int axis = -1;   // 0/1/2 when the static normal is exactly that unit axis (kernel specialisation)
    int frames_per_stage = kFramesPerStage;   // G = 4 frames staged per pass (8 was measured at 26 % and spilled: removed in round 4)
    bool membrane_is_frame = false;            // the membrane group is every atom of the frame, in order
    uint32_t wg_capacity = 256u * 6u;          // co-resident workgroups of the tiled kernel on this device
    uint32_t lw = 0;
    size_t lds_bytes = 0;
    uint64_t n_frames = 0;
    uint64_t err_index = 0;
    std::string err_msg;
    // kernel timing (gorder_hip_kernel_time / _group): OFF until the host asks for it once.  Everything a handle queues
    // runs in order on ONE stream, so a submit is a chain of labelled segments between events E0 [leaflet kernels] E1
    // [order kernels] E2 ... En: timing_mark(label) closes the open segment with a new event and opens the next.  The
    // events are a fixed ring, drained (oldest segment first) when it runs low — nothing grows with the trajectory.
    static constexpr uint32_t kTimingEvents = 1024;
    struct TimingSeg { uint32_t label, ev_a, ev_b; };
    bool timing_on = false;
    Event timing_ev[kTimingEvents];
    uint32_t timing_next_ev = 0;                  // ring position of the next event to record
    int timing_open_label = -1;                   // the segment being queued (-1: none)
    uint32_t timing_open_ev = 0;
    std::deque<TimingSeg> timing_pending;         // closed segments whose events have not been read yet
    std::vector<std::string> timing_labels;       // group names in order of first appearance since the last reset
    std::vector<double> timing_label_ms;
    std::vector<uint64_t> timing_label_n;
    uint64_t timing_launches = 0;                 // submits (chains) since the last reset
    std::string timed_kernels;                    // the labels joined by " + " (gorder_hip_kernel_time_names)
    // host copies behind the payload of gorder_hip_last_error_index
    std::vector<uint32_t> host_heads, host_dyn_heads;
    DBuf<uint32_t> d_mol_slot0;
    uint64_t err_frame = 0;
    // frame indices of the batches submitted since the last clean synchronisation (ordinal -> SystemTopology::frame of
    // its frames), so that a device error names the frame of the TRAJECTORY; arithmetic progressions are kept as three
    // numbers, at most kBatchLog batches are remembered
    struct BatchLog { uint64_t ordinal, first, stride; std::vector<uint64_t> list; };
    static constexpr size_t kBatchLog = 4096;
    std::deque<BatchLog> batch_log;
    uint64_t n_submits = 0;
    const unsigned long long *decoder_key = nullptr;   // gorder_hip_run_trajectory: the slot's decoder record, for the next submit only
    // collected history (gorder_hip_set_collect): per batch the rows are packed into a device staging block (k_collect_flags,
    // k_collect_normals) and copied, stream-ordered, into the pinned chunks of the stores (collect_store.h)
    uint32_t collect = 0;                       // gorder_collect_t bits
    bool collect_locked = false;                // something was submitted or primed since create / reset
    gorder::CollectStore collect_flags;         // rows of ceil(n_mol / 64) u64
    gorder::CollectStore collect_normals;       // rows of n_mol x 3 f32
    DBuf<u64> d_collect_words;
    DBuf<CollectVec3> d_collect_vec;
    DBuf<uint8_t> d_touched;                    // [n_frames][n_mol_total] of the batch (ExtraArgs::touched)
    // whole-trajectory manual tables (gorder_hip_set_manual_leaflet_table / _normal_table; replay_rows.h): packed on the
    // device, expanded per batch by k_replay_flags / k_replay_normals
    DBuf<u64> d_ltable;                         // [window rows][ceil(n_mol / 64)] u64, before `flip`
    gorder::ReplayWindow ltable_win;
    bool replay_have_carry = false;             // row 0 of d_aflags is the table's row replay_carry_index
    uint64_t replay_carry_index = 0;
    DBuf<ReplayVec3> d_ntable;                  // [window rows][n_mol] x 12 bytes
    gorder::ReplayWindow ntable_win;
    uint32_t ntable_step = 1;
    DBuf<uint32_t> d_nrow;                      // per frame of the batch: its row of d_ntable
    // radial shells (gorder_hip_set_radial_shells; kernels_radial.h): the accumulators [n_shells][4][n_acc] laid out like d_acc,
    // their replicas [shells.n_rep][n_shells][4][n_acc] (k_bonds_shells adds into them)
    uint32_t n_shells = 0;
    float shell_thr[GORDER_RADIAL_MAX_SHELLS] = {};          // local_radius_threshold of the radii
    RepAcc shells;
    size_t shell_lds_bytes = 0;                 // the LDS table of the widest tile
    bool shell_direct = false;                  // per-sample global atomics: the table does not fit, or GORDER_HIP_RADIAL_DIRECT
    // order distributions (gorder_hip_set_order_histogram; kernels_hist.h): the counts [n_bins][2][n_acc] (total, upper), their
    // replicas [hist.n_rep][n_bins][2][n_acc] (k_bonds_dist adds into them), the edges on the device
    uint32_t hist_edges = 0;                    // n_edges, 0 = off
    DBuf<int32_t> d_hist_edges;
    RepAcc hist;
    size_t hist_table_words = 0;                // the LDS table of the widest tile, in u32 words
    bool hist_direct = false;                   // per-sample global atomics: the table does not fit, or GORDER_HIP_DIST_DIRECT
    BondCorr corr;
    NeighbourClasses nb;
    // per-molecule rows (gorder_hip_set_molecule_rows; molecule_rows.h, kernels_molrows.h): the lane order and the run tables,
    // the staging block of one frame sub-range [frames][n_groups][n_mol_total] packed words, and the rows in pinned chunks
    gorder::MolRows mol;                        // mol.n_groups != 0: the rows are on
    DBuf<Item> d_mol_items;
    DBuf<gorder::MolRun> d_mol_runs;
    DBuf<uint32_t> d_mol_run_begin;
    gorder::UaMolRows ua_mol;                   // GORDER_FLAG_UA_SAMPLES: the united-atom tiles' word lists (ua_molecule_rows.h; k_ua_mol)
    DBuf<gorder::UaLaneWords> d_ua_mol_lanes;
    DBuf<uint32_t> d_ua_mol_words, d_ua_mol_word_begin;
    DBuf<u64> d_mol_stage;
    gorder::CollectStore mol_store;             // rows of n_groups x n_mol_total u64
    const uint64_t *mol_frame_index = nullptr;  // the batch being submitted: its frames' labels
    bool mol_failed = false;                    // a device error ended the run: its batch and the later ones append nothing
    std::deque<std::pair<uint64_t, uint64_t>> mol_batch_log;   // (batch ordinal, rows before it), as batch_log
};

namespace {

int fail(gorder_hip_handle *h, int status, const std::string &msg) {
    if (h) h->err_msg = msg;
    return status;
}

#define HIP_TRY(h, expr)                                                                    \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
            return fail(h, GORDER_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

#define ST_TRY(expr)                                \
    do {                                            \
        const int st_ = (expr);                     \
        if (st_ != GORDER_OK) return st_;           \
    } while (0)

// an allocation a policy of device_mem.h refused, as a status with HIP's words for it (reading the error clears it: the
// handle stays usable)
int alloc_failed(gorder_hip_handle *h, const char *call) {
    return fail(h, GORDER_ERR_DEVICE, std::string(call) + ": " + hipGetErrorString(hipGetLastError()));
}

// exactly n elements; with `fill` every byte of them set to it (null stream: gorder_hip_create waits for the device at its end)
template <typename T, typename Mem>
int allocate(gorder_hip_handle *h, gorder::Buf<T, Mem> &dst, size_t n, int fill = -1) {
    if (!dst.alloc(n)) return alloc_failed(h, std::is_same<Mem, DeviceMem>::value ? "hipMalloc" : "hipHostMalloc");
    if (fill >= 0 && n) HIP_TRY(h, hipMemset(dst, fill, n * sizeof(T)));
    return GORDER_OK;
}

template <typename T>
int upload(gorder_hip_handle *h, DBuf<T> &dst, const std::vector<T> &src) {
    ST_TRY(allocate(h, dst, src.size()));
    if (!src.empty()) HIP_TRY(h, hipMemcpy(dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return GORDER_OK;
}

// room for `need` elements, contents not kept (Buf::reserve); *grew: the block is a new one and holds nothing yet
template <typename T>
int ensure(gorder_hip_handle *h, DBuf<T> &buf, size_t need, bool *grew = nullptr) {
    const gorder::Reserve r = buf.reserve(need);
    if (grew) *grew = r == gorder::Reserve::Grew;
    return r == gorder::Reserve::Failed ? alloc_failed(h, "hipMalloc") : GORDER_OK;
}

// an accumulator block of `words` words and its replicas (as many as the ordinary sums have, gorder::replica_count), zeroed
// in the order of the handle's stream
int alloc_zeroed(gorder_hip_handle *h, RepAcc &r, size_t words) {
    if (!r.alloc(words, h->sw.replicas)) {
        r.reset();
        return alloc_failed(h, "hipMalloc");
    }
    HIP_TRY(h, r.zero_async(h->stream));
    return GORDER_OK;
}

// (slot, molecule, which atom) of an order sample -> atom index in the frame (the payload of UndefinedPosition,
// errors.rs:136).  Error path only: a linear walk over the plan.
uint32_t sample_atom(const Plan &p, uint32_t slot, uint32_t mol, uint32_t which) {
    for (const Tile &t : p.tiles)
        for (uint32_t q = 0; q < t.n_items; q++) {
            const Item &it = p.items[t.item0 + q];
            if (it.mol == mol && p.tile_slots[t.slot0 + it.lslot] == slot) return t.atom0 + (which ? it.lj : it.li);
        }
    for (const DirectItem &d : p.direct)
        if (d.mol == mol && d.slot == slot) return which ? d.j : d.i;
    for (const Tile &t : p.ua_tiles)
        for (uint32_t q = 0; q < t.n_items; q++) {
            const gorder::UaItem &it = p.ua_items[t.item0 + q];
            if (it.mol == mol && p.ua_tile_slots[t.slot0 + it.lslot0] == slot) return t.atom0 + it.l[which & 3u];
        }
    return 0;
}

// Decode the device's error key (kernels_common.h, raise_error): status, frame, payload.
int check_device_error(gorder_hip_handle *h) {
    unsigned long long rec[3] = {kErrNone, kErrNone, 0};
    HIP_TRY(h, hipMemcpy(rec, h->d_err, sizeof(rec), hipMemcpyDeviceToHost));
    // [1]: latched at the end of a batch; [0]: raised outside a batch (priming frame, stand-alone decode) and not committed yet
    const bool latched = rec[1] != kErrNone;
    const unsigned long long key = latched ? rec[1] : rec[0];
    if (key == kErrNone) { h->batch_log.clear(); h->mol_batch_log.clear(); return GORDER_OK; }
    if (latched && !h->mol_failed)      // per-molecule rows: the batch that raised it and the later ones leave no rows (the stream is idle here)
        if (h->mol.n_groups && !h->mol_batch_log.empty()) {
            // (a batch older than the log keeps kBatchLog entries of: the rows are cut at the oldest batch still known, which
            // is later than the failed one — rows are lost, none of a failed batch is kept)
            uint64_t keep = h->mol_batch_log.front().second;
            for (const auto &b : h->mol_batch_log)
                if (b.first <= rec[2]) keep = b.second;
            if (rec[2] > h->mol_batch_log.back().first) keep = h->mol_store.n_rows();      // (raised by a batch without rows)
            h->mol_store.truncate(keep);
            h->mol_failed = true;
        }
    const uint32_t code = (uint32_t)(key & 15u), detail = (uint32_t)(key >> 4) & 3u, mol = (uint32_t)(key >> 6) & 0x1ffffu;
    const uint32_t sample = (uint32_t)(key >> 23) & 1u, slot = (uint32_t)(key >> 24) & 0x3fffu;
    const uint32_t stage = (uint32_t)(key >> 38) & 3u, frame = (uint32_t)(key >> 40) & 0x7fffffu;
    const int status = code == 8u ? (int)GORDER_ERR_BOX_RANGE : (code == 9u ? (int)GORDER_ERR_TRAJECTORY_FORMAT :
                       (code == 10u ? (int)GORDER_ERR_CLUSTERING : (code == 11u ? (int)GORDER_ERR_CLUSTER_MATCH : (int)code)));
    h->err_frame = frame;
    char where[96];
    snprintf(where, sizeof(where), "frame %u of a batch", frame);
    if (latched)
        for (const auto &b : h->batch_log)
            if (b.ordinal == rec[2]) {
                if (b.list.empty()) h->err_frame = b.first + (uint64_t)frame * b.stride;
                else if (frame < b.list.size()) h->err_frame = b.list[frame];
                snprintf(where, sizeof(where), "frame %llu of the trajectory (frame %u of batch %llu)",
                         (unsigned long long)h->err_frame, frame, (unsigned long long)rec[2]);
                break;
            }
    h->err_index = 0;
    if (status == GORDER_ERR_UNDEFINED_POSITION) {
        if (stage == kStageTypes && sample) h->err_index = sample_atom(h->plan, slot, mol, detail);
        else if (h->nb.on() && stage == kStageSystem) {      // k_neighbour_counts: a molecule's centre, or a position in the neighbour list
            const std::vector<uint32_t> &atoms = detail ? h->nb.neighbours : h->nb.centres;
            if (mol < atoms.size()) h->err_index = atoms[mol];
        }
        else if (mol < h->host_dyn_heads.size()) h->err_index = h->host_dyn_heads[mol];   // head of a dynamic-normal cloud
    } else if (status == GORDER_ERR_INVALID_LOCAL_MEMBRANE_CENTER) {
        if (mol < h->host_heads.size()) h->err_index = h->host_heads[mol];                // leaflets.rs:661-675: the head's index
    } else if (status == GORDER_ERR_DYNAMIC_NORMAL) {
        h->err_index = detail;                                                             // NotEnoughPoints(n)
    } else if (status == GORDER_ERR_CLUSTERING || status == GORDER_ERR_CLUSTER_MATCH) {
        h->err_index = h->err_frame;                                                       // the frame whose distances are not finite
    }
    char buf[200];
    snprintf(buf, sizeof(buf), "device raised %s (payload %llu) in %s", gorder_hip_strerror(status),
             (unsigned long long)h->err_index, where);
    h->err_msg = buf;
    return status;
}

// ---- kernel timing: labelled segments between events on the handle's stream (see gorder_hip_handle::timing_ev) -----
int timing_drain_oldest(gorder_hip_handle *h) {
    const gorder_hip_handle::TimingSeg sg = h->timing_pending.front();
    float t = 0.0f;
    HIP_TRY(h, hipEventSynchronize(h->timing_ev[sg.ev_b]));
    HIP_TRY(h, hipEventElapsedTime(&t, h->timing_ev[sg.ev_a], h->timing_ev[sg.ev_b]));
    h->timing_label_ms[sg.label] += t;
    h->timing_label_n[sg.label] += 1;
    h->timing_pending.pop_front();
    return GORDER_OK;
}
// Close the open segment (if any) at a new event and, with a label, open the next one there.  No-op while timing is off.
int timing_mark(gorder_hip_handle *h, const char *label) {
    if (!h->timing_on) return GORDER_OK;
    if (!label && h->timing_open_label < 0) return GORDER_OK;
    // a pending segment holds at most two events of the ring: keep fewer than half of it pending
    while (h->timing_pending.size() >= gorder_hip_handle::kTimingEvents / 2u - 2u) {
        ST_TRY(timing_drain_oldest(h));
    }
    const uint32_t ev = h->timing_next_ev;
    h->timing_next_ev = (ev + 1u) % gorder_hip_handle::kTimingEvents;
    HIP_TRY(h, h->timing_ev[ev].create(hipEventDefault));
    HIP_TRY(h, hipEventRecord(h->timing_ev[ev], h->stream));
    if (h->timing_open_label >= 0) h->timing_pending.push_back({(uint32_t)h->timing_open_label, h->timing_open_ev, ev});
    h->timing_open_label = -1;
    if (label) {
        size_t k = 0;
        while (k < h->timing_labels.size() && h->timing_labels[k] != label) k++;
        if (k == h->timing_labels.size()) {
            h->timing_labels.push_back(label);
            h->timing_label_ms.push_back(0.0);
            h->timing_label_n.push_back(0);
            if (!h->timed_kernels.empty()) h->timed_kernels += " + ";
            h->timed_kernels += label;
        }
        h->timing_open_label = (int)k;
        h->timing_open_ev = ev;
    }
    return GORDER_OK;
}
#define TIMING_MARK(h, label)                                   \
    do {                                                        \
        const int tm_ = timing_mark(h, label);                  \
        if (tm_ != GORDER_OK) return tm_;                       \
    } while (0)

// Launch the order kernels of one batch (internal).
// fold the replicas into the accumulator block (stream-ordered; cheap: 4 * n_acc threads)
int fold_replicas(gorder_hip_handle *h) {
    if (!h->rep_dirty || !h->d_rep) return GORDER_OK;
    const uint32_t n = 4u * h->plan.n_acc;
    hipLaunchKernelGGL(k_fold_replicas, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->d_acc, h->d_rep, h->sw.replicas, n);
    HIP_TRY(h, hipGetLastError());
    h->rep_dirty = false;
    return GORDER_OK;
}

// unpack the ordermap words the scatter kernels filled since the last fold (k_fold_maps)
int fold_maps(gorder_hip_handle *h) {
    if (!h->extra.maps || !h->map_pending) return GORDER_OK;
    const size_t n = (size_t)h->plan.n_acc * h->map_nx * h->map_ny;
    const uint32_t blocks = (uint32_t)std::min<size_t>((n + 255) / 256, 256 * 16);
    hipLaunchKernelGGL(k_fold_maps, dim3(blocks), dim3(256), 0, h->stream, h->d_map_packed, h->d_map_sums, h->d_map_cnts,
                       n, h->tables.leaflets.method != GORDER_LEAFLETS_NONE ? 1 : 0);
    HIP_TRY(h, hipGetLastError());
    h->map_pending = 0;
    return GORDER_OK;
}

// the cell list of `ns` slab frames (k_local_build, or bin / scan / scatter for very large atom sets); `counts` are the
// lo.cell_count and lo.cell_fill words the three-kernel form needs zeroed
int launch_cell_list(gorder_hip_handle *h, const LocalArgs &lo, uint32_t ns, uint32_t n_list, void *counts, size_t count_bytes) {
    const bool three = h->sw.local_three_kernels;    // GORDER_HIP_LOCAL_THREE_KERNELS, an A/B switch; also what membranes beyond kLocalBuildMax take
    TIMING_MARK(h, n_list <= kLocalBuildMax && !three ? "k_local_build" : "k_local_bin + k_local_scan + k_local_scatter");
    if (n_list <= kLocalBuildMax && !three) {
        // (a thread keeps a byte per atom it places: the kernel compiled for 2, 5 or 8 trips of eight atoms per thread)
        if (n_list <= 2u * 8192u) hipLaunchKernelGGL(k_local_build<2>, dim3(ns), dim3(1024), kLocalBuildLds, h->stream, lo);
        else if (n_list <= 5u * 8192u) hipLaunchKernelGGL(k_local_build<5>, dim3(ns), dim3(1024), kLocalBuildLds, h->stream, lo);
        else hipLaunchKernelGGL(k_local_build<kLocalBuildTrips>, dim3(ns), dim3(1024), kLocalBuildLds, h->stream, lo);
        return GORDER_OK;
    }
    HIP_TRY(h, hipMemsetAsync(counts, 0, count_bytes, h->stream));
    const dim3 ga((n_list + 255) / 256, ns);
    hipLaunchKernelGGL(k_local_bin, ga, dim3(256), 0, h->stream, lo);
    hipLaunchKernelGGL(k_local_scan, dim3(ns), dim3(1024), 0, h->stream, lo);
    hipLaunchKernelGGL(k_local_scatter, ga, dim3(256), 0, h->stream, lo);
    return GORDER_OK;
}

// normals of every molecule for the frames of this batch -> h->d_dyn_normals [n_frames][n_mol_total]
int run_dynamic_normals(gorder_hip_handle *h, const FrameArgs &a) {
    int st;
    const uint32_t n_mol = h->plan.n_mol_total;
    if ((st = ensure(h, h->d_dyn_normals, (size_t)a.n_frames * n_mol)) != GORDER_OK) return st;
    const gorder_dynamic_normal_t &dn = h->tables.dynamic_normal;
    const size_t ncell = (size_t)kLocalMaxCells1D * kLocalMaxCells1D;
    LocalArgs lo{};
    lo.xyz = a.xyz; lo.box9 = a.box9; lo.n_atoms = a.n_atoms;
    lo.n_mol_total = n_mol; lo.heads = h->d_dyn_heads; lo.membrane = h->d_dyn_cloud; lo.n_membrane = dn.n_cloud;
    lo.dim = 2; lo.pbc = a.pbc; lo.radius = dn.radius; lo.radius_thr = local_radius_threshold(dn.radius);
    lo.halo = 0; lo.rec_stride = dn.n_cloud;
    lo.cell_of = h->d_dyn_cell_of; lo.trig = h->d_dyn_rec;
    lo.cell_count = h->d_dyn_count; lo.cell_fill = h->d_dyn_count + h->dyn_slab * (ncell + 1);
    lo.err = h->d_err; lo.aframes = nullptr; lo.write_dist_frame = -1;
    for (uint32_t done = 0; done < a.n_frames; done += h->dyn_slab) {
        const uint32_t ns = std::min(a.n_frames - done, h->dyn_slab);
        lo.frame0 = done;
        lo.n_slab = ns;
        if ((st = launch_cell_list(h, lo, ns, dn.n_cloud, h->d_dyn_count,
                                   (size_t)h->dyn_slab * (2 * ncell + 1) * sizeof(uint32_t))) != GORDER_OK) return st;
        TIMING_MARK(h, "k_dyn_cov + k_dyn_eigen");
        hipLaunchKernelGGL(k_dyn_cov, dim3((n_mol + 15) / 16, ns), dim3(256), 0, h->stream, lo, h->d_dyn_cov);
        hipLaunchKernelGGL(k_dyn_eigen, dim3((uint32_t)(((size_t)ns * n_mol + 255) / 256)), dim3(256), 0, h->stream, lo, h->d_dyn_cov,
                           h->d_dyn_normals);
    }
    HIP_TRY(h, hipGetLastError());
    // keep the last frame's normals for gorder_hip_normals (stream-ordered copy into pageable memory)
    h->last_normals.resize(4 * (size_t)n_mol);
    HIP_TRY(h, hipMemcpyAsync(h->last_normals.data(), h->d_dyn_normals + (size_t)(a.n_frames - 1) * n_mol,
                              4 * sizeof(float) * (size_t)n_mol, hipMemcpyDeviceToHost, h->stream));
    return GORDER_OK;
}

// ---- runtime values as template arguments: f(std::integral_constant<int, V>{}) for the V among Vs... that equals v (the
// last one where none does), so that one generic lambda holds the launch expression of a whole kernel family
template <int V, int... Vs, class F>
void with_int(int v, F &&f) {
    if constexpr (sizeof...(Vs) > 0) { if (v != V) return with_int<Vs...>(v, f); }
    f(std::integral_constant<int, V>{});
}
template <class F> void with_bool(bool v, F &&f) { if (v) f(std::true_type{}); else f(std::false_type{}); }
template <class F> void with_axis(int axis, F &&f) { with_int<2, 1, 0, -1>(axis, f); }
template <class F> void with_npf(int npf, F &&f) { with_int<4, 5>(npf, f); }
static_assert(gorder::kStageFrames == kRecFrames && gorder::kStageFrames == (uint32_t)kFramesPerStage, "order_route.h: frames of a stage");
// the grid of the united-atom tile kernels: a workgroup per (chunk, tile), padded to a multiple of 8 (ua_tile_work, kernels_ua.h)
uint64_t ua_grid(uint32_t n_tiles, uint32_t n_chunks) { return ((uint64_t)n_tiles * n_chunks + 7u) / 8u * 8u; }

// k_bonds_tiled_mol over the frames of the batch, in sub-ranges the staging block holds: zero the block, run the order pass,
// queue the copy of the sub-range's rows into the pinned chunks — stream-ordered, nothing waits
int collect_copy_out(gorder_hip_handle *h, gorder::CollectStore &store, const void *d_block, const uint64_t *frames, size_t n_rows);
int launch_molecule_rows(gorder_hip_handle *h, const FrameArgs &a, const gorder::OrderRoute &route) {
    const Plan &p = h->plan;
    const bool bonds = route.family == gorder::BondFamily::TiledMol, ua = route.ua_kernel == gorder::UaKernel::Mol;
    const uint32_t n_tiles = (uint32_t)p.tiles.size(), n_ua = (uint32_t)p.ua_tiles.size();
    const bool ac = (h->tables.flags & GORDER_FLAG_TRIG_ACOS_COS) != 0;
    const size_t wpf = (size_t)h->mol.n_groups * p.n_mol_total;
    const uint32_t sub = gorder::molecule_rows_subrange(a.n_frames, wpf, h->sw.mol_rows_staging);      // (GORDER_HIP_MOL_ROWS_STAGING)
    int st;
    if ((st = ensure(h, h->d_mol_stage, wpf * sub)) != GORDER_OK) return st;
    MolRowArgs mr{};
    mr.runs = h->d_mol_runs; mr.run_begin = h->d_mol_run_begin; mr.stage = h->d_mol_stage; mr.words_per_frame = (uint32_t)wpf;
    UaMolArgs um{};
    um.word_begin = h->d_ua_mol_word_begin; um.words = h->d_ua_mol_words; um.lane_words = h->d_ua_mol_lanes; um.stage = h->d_mol_stage;
    um.words_per_frame = (uint32_t)wpf; um.list_bytes = (uint32_t)gorder::ua_mol_list_bytes(h->ua_mol.max_local);
    um.n_buf = gorder::ua_mol_buffers(h->ua_mol.max_local);
    const ExtraArgs e = h->extra;       // (the hydrogen construction's constants and the axis; no geometry, maps or rows: the setter refuses them)
    for (uint32_t lo = 0; lo < a.n_frames; lo += sub) {
        const uint32_t hi = std::min(a.n_frames, lo + sub), nf = hi - lo;
        FrameArgs b = a;
        b.frame0 = lo; b.n_frames = hi;
        TIMING_MARK(h, bonds ? route.label : "k_ua_mol");
        HIP_TRY(h, hipMemsetAsync(h->d_mol_stage, 0, wpf * nf * sizeof(unsigned long long), h->stream));
        if (bonds) {
            const gorder::FrameChunks c = gorder::extras_chunks(nf, n_tiles, h->sw.wg_target, h->wg_capacity, false, true);
            const uint64_t grid = (uint64_t)n_tiles * c.n_chunks;
            if (grid > 0x7fffffffull) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "batch too large");
            b.frames_per_chunk = c.frames_per_chunk;
            const dim3 g((uint32_t)grid), blk(kBlock);
            with_npf(route.npf, [&](auto NPF) { with_bool(b.pbc, [&](auto PBC) { with_bool(b.leaflets, [&](auto LF) {
                if (ac)     // (the literal cosine: the general normal's code for every axis)
                    hipLaunchKernelGGL((k_bonds_tiled_mol<NPF(), true, PBC(), LF(), -1>), g, blk, h->lds_bytes, h->stream, b, mr, b.xyz, b.box9,
                                       b.aflags, b.arow, h->d_tiles, h->d_mol_items, h->d_tile_slots, n_tiles, h->lw);
                else with_int<2, -1>(h->axis, [&](auto AX) {      // (a normal along z, or the general code: exact for x and y as well)
                    hipLaunchKernelGGL((k_bonds_tiled_mol<NPF(), false, PBC(), LF(), AX()>), g, blk, h->lds_bytes, h->stream, b, mr, b.xyz, b.box9,
                                       b.aflags, b.arow, h->d_tiles, h->d_mol_items, h->d_tile_slots, n_tiles, h->lw);
                });
            }); }); });
            HIP_TRY(h, hipGetLastError());
        }
        if (ua) {       // the united-atom tiles add into the same block (GORDER_FLAG_UA_SAMPLES)
            const gorder::FrameChunks c = gorder::extras_chunks(nf, n_ua, h->sw.wg_target, h->wg_capacity, false, true);
            const uint64_t grid = ua_grid(n_ua, c.n_chunks);
            if (grid > 0x7fffffffull) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "batch too large");
            b.frames_per_chunk = c.frames_per_chunk;
            if (bonds) TIMING_MARK(h, "k_ua_mol");
            with_bool(ac, [&](auto AC) {
                hipLaunchKernelGGL((k_ua_mol<AC()>), dim3((uint32_t)grid), dim3(kBlock), gorder::ua_mol_lds_bytes(h->ua_mol.max_local), h->stream, b, e,
                                   um, b.xyz, b.box9, b.aflags, b.arow, h->d_ua_tiles, h->d_ua_items, h->d_ua_tile_slots, n_ua);
            });
            HIP_TRY(h, hipGetLastError());
        }
        if ((st = collect_copy_out(h, h->mol_store, h->d_mol_stage, h->mol_frame_index + lo, nf)) != GORDER_OK) return st;
    }
    return GORDER_OK;
}

// ---- the order kernels of one batch, as `route` has them: launch_orders, at the end of this section, is the dispatcher; every
// kernel group opens a timing segment of its own.  A combination of template arguments without a kernel (`if constexpr`) is
// one the route never asks for: tests/test_order_route_cpu.py.
bool literal_cosine(const gorder_hip_handle *h) { return (h->tables.flags & GORDER_FLAG_TRIG_ACOS_COS) != 0; }

// the shape of the geometry selection in every frame of the batch -> h->d_shapes
int launch_geometry_shapes(gorder_hip_handle *h, const FrameArgs &a) {
    ST_TRY(ensure(h, h->d_shapes, (size_t)a.n_frames * 8));
    const gorder_geometry_t &ge = h->tables.geometry;
    GeomArgs ga{};
    ga.xyz = a.xyz; ga.box9 = a.box9; ga.n_atoms = a.n_atoms; ga.pbc = a.pbc;
    ga.kind = ge.kind; ga.reference = ge.reference; ga.orientation = ge.orientation;
    for (int d = 0; d < 3; d++) { ga.point[d] = ge.point[d]; ga.structure_box[d] = ge.structure_box[d]; }
    for (int d = 0; d < 2; d++) { ga.xdim[d] = ge.xdim[d]; ga.ydim[d] = ge.ydim[d]; ga.zdim[d] = ge.zdim[d]; ga.span[d] = ge.span[d]; }
    ga.radius = ge.radius; ga.group = h->d_geom_group; ga.n_group = ge.n_group;
    ga.shapes = h->d_shapes; ga.err = h->d_err;
    TIMING_MARK(h, "k_geom_shapes");
    hipLaunchKernelGGL(k_geom_shapes, dim3(a.n_frames), dim3(256), 0, h->stream, ga);
    HIP_TRY(h, hipGetLastError());
    return GORDER_OK;
}

// Tiled and Gather: one launch over the whole batch (its chunking stays in `a`)
int launch_tiled(gorder_hip_handle *h, FrameArgs &a, const gorder::OrderRoute &route) {
    const uint32_t n_tiles = (uint32_t)h->plan.tiles.size();
    const gorder::FrameChunks c = gorder::tiled_chunks(a.n_frames, (uint32_t)h->frames_per_stage, n_tiles, h->sw.wg_target, h->wg_capacity);
    a.frames_per_chunk = c.frames_per_chunk;
    const uint64_t grid = (uint64_t)n_tiles * c.n_chunks;
    if (grid > 0x7fffffffull) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "batch too large");
    const dim3 g((uint32_t)grid), b(kBlock);
    TIMING_MARK(h, route.label);
    with_bool(literal_cosine(h), [&](auto AC) { with_bool(a.pbc, [&](auto PBC) { with_bool(a.leaflets, [&](auto LF) {
        if (route.family == gorder::BondFamily::Gather)
            hipLaunchKernelGGL((k_bonds_gather<4, AC(), PBC(), LF()>), g, b, 0, h->stream, a, a.xyz, a.box9, a.aflags, a.arow,
                               h->d_tiles, h->d_items, h->d_tile_slots, n_tiles);
        else with_npf(route.npf, [&](auto NPF) { with_axis(h->axis, [&](auto AX) { with_bool(route.mom, [&](auto MOM) {
            if constexpr (LF() || !MOM())
                hipLaunchKernelGGL((k_bonds_tiled<4, NPF(), AC(), PBC(), LF(), AX(), MOM()>), g, b, h->lds_bytes, h->stream, a,
                                   a.xyz, a.box9, a.aflags, a.arow, h->d_tiles, h->d_items, h->d_tile_slots, n_tiles, h->lw);
        }); }); });
    }); }); });
    HIP_TRY(h, hipGetLastError());
    return GORDER_OK;
}

// One sub-range [lo, hi) of the batch's frames in the loop of the scatter-bound kernels: what its passes are handed
struct SubRange {
    const FrameArgs &a;                 // the batch
    const gorder::OrderRoute &route;
    uint32_t lo, hi;
    bool class_rows_whole;              // neighbour classes: the class rows hold the whole batch, not this sub-range alone
    uint32_t nf() const { return hi - lo; }
    FrameArgs frames(const gorder::FrameChunks &c) const {      // the batch's arguments narrowed to the sub-range, cut as `c` says
        FrameArgs b = a;
        b.frame0 = lo; b.n_frames = hi; b.frames_per_chunk = c.frames_per_chunk;
        return b;
    }
};
const Item *bond_items(const gorder_hip_handle *h, const gorder::OrderRoute &route) { return route.items_by_slot ? h->d_items_by_slot : h->d_items; }

// the class of every (frame, molecule) of the sub-range (k_neighbour_counts, a frame per row of gridDim.y), then the kernel that reads it
int launch_classes(gorder_hip_handle *h, const SubRange &s) {
    const Plan &p = h->plan;
    NeighbourClasses &nb = h->nb;
    const uint32_t nt = (uint32_t)p.tiles.size(), nf = s.nf();
    const gorder::FrameChunks c = gorder::shells_chunks(nf, nt, h->sw.wg_target, h->wg_capacity, kShellChunkMax);
    FrameArgs b = s.frames(c);
    ClassArgs ca{};
    ca.centres = nb.d_centres; ca.neighbours = nb.d_neighbours; ca.n_neighbours = (uint32_t)nb.neighbours.size();
    ca.thr = nb.thr; ca.n = nb.n_classes; ca.rows = nb.rows; ca.row_base = s.class_rows_whole ? 0u : s.lo;
    ca.axis = h->axis; ca.rep = nb.acc.rep; ca.n_rep = nb.acc.n_rep;
    nb.rows_frames = s.class_rows_whole ? s.a.n_frames : nf;
    TIMING_MARK(h, "k_neighbour_counts");
    hipLaunchKernelGGL(k_neighbour_counts, dim3((p.n_mol_total + 255u) / 256u, nf), dim3(256), 0, h->stream, ca, b.xyz, b.box9,
                       b.n_atoms, p.n_mol_total, b.pbc, s.lo, h->d_err);
    TIMING_MARK(h, s.route.label);
    // the table of the widest tile, or the [2][256] u64 + [2][256] u32 of the direct route's reduction
    const size_t lds = nb.direct ? (size_t)kBlock * 24u : nb.lds_bytes;
    with_bool(literal_cosine(h), [&](auto AC) { with_bool(nb.direct, [&](auto DIRECT) {
        hipLaunchKernelGGL((k_bonds_classes<AC(), DIRECT()>), dim3(nt * c.n_chunks), dim3(kBlock), lds, h->stream, b, ca, b.xyz, b.box9,
                           b.aflags, b.arow, h->d_tiles, bond_items(h, s.route), h->d_tile_slots, nt);
    }); });
    return GORDER_OK;
}

int launch_shells(gorder_hip_handle *h, const SubRange &s, const ExtraArgs &e) {
    const uint32_t nt = (uint32_t)h->plan.tiles.size();
    const gorder::FrameChunks c = gorder::shells_chunks(s.nf(), nt, h->sw.wg_target, h->wg_capacity, kShellChunkMax);
    FrameArgs b = s.frames(c);
    ShellArgs sa{};
    sa.n = h->n_shells; sa.rep = h->shells.rep; sa.n_rep = h->shells.n_rep;
    for (uint32_t k = 0; k < GORDER_RADIAL_MAX_SHELLS; k++) sa.thr[k] = k < h->n_shells ? h->shell_thr[k] : INFINITY;
    // the table of the widest tile, or the [2][256] u64 + [2][256] u32 of the direct route's reduction
    const size_t lds = h->shell_direct ? (size_t)kBlock * 24u : h->shell_lds_bytes;
    TIMING_MARK(h, s.route.label);
    with_bool(literal_cosine(h), [&](auto AC) { with_bool(h->shell_direct, [&](auto DIRECT) {
        hipLaunchKernelGGL((k_bonds_shells<AC(), DIRECT()>), dim3(nt * c.n_chunks), dim3(kBlock), lds, h->stream, b, e, sa, b.xyz, b.box9,
                           b.aflags, b.arow, h->d_tiles, bond_items(h, s.route), h->d_tile_slots, nt);
    }); });
    return GORDER_OK;
}

int launch_dist(gorder_hip_handle *h, const SubRange &s, const ExtraArgs &e) {
    const uint32_t nt = (uint32_t)h->plan.tiles.size();
    const gorder::FrameChunks c = gorder::dist_chunks(s.nf(), nt, h->sw.wg_target, h->wg_capacity, h->hist_direct ? 0u : (uint32_t)h->hist_table_words,
                                                      h->sw.dist_samples_per_word, kDistChunkMax);
    FrameArgs b = s.frames(c);
    DistArgs da{};
    da.n_edges = h->hist_edges; da.edges = h->d_hist_edges; da.rep = h->hist.rep; da.n_rep = h->hist.n_rep;
    // the edges, then the table of the widest tile or the ordinary sums' reduction, whichever is larger
    const size_t lds = kDistEdgeBytes + std::max<size_t>(kDistReduceBytes, h->hist_direct ? 0u : h->hist_table_words * sizeof(uint32_t));
    TIMING_MARK(h, s.route.label);
    with_bool(literal_cosine(h), [&](auto AC) { with_bool(h->hist_direct, [&](auto DIRECT) {
        hipLaunchKernelGGL((k_bonds_dist<AC(), DIRECT()>), dim3(nt * c.n_chunks), dim3(kBlock), lds, h->stream, b, e, da, b.xyz, b.box9,
                           b.aflags, b.arow, h->d_tiles, bond_items(h, s.route), h->d_tile_slots, nt);
    }); });
    return GORDER_OK;
}

// scatter-bound modes: the plain per-sample kernel (see "Extras" above)
int launch_extras(gorder_hip_handle *h, const SubRange &s, const ExtraArgs &e) {
    const uint32_t nt = (uint32_t)h->plan.tiles.size();
    const gorder::FrameChunks c = gorder::extras_chunks(s.nf(), nt, h->sw.wg_target, h->wg_capacity, s.route.map_accumulate, false);
    FrameArgs b = s.frames(c);
    TIMING_MARK(h, s.route.label);
    with_bool(literal_cosine(h), [&](auto AC) { with_bool(s.route.maps_only, [&](auto MO) {
        hipLaunchKernelGGL((k_bonds_extras<AC(), MO()>), dim3(nt * c.n_chunks), dim3(kBlock), 0, h->stream, b, e, b.xyz, b.box9, b.aflags,
                           b.arow, h->d_tiles, bond_items(h, s.route), h->d_tile_slots, nt);
    }); });
    return GORDER_OK;
}

// TiledTw and TiledMaps: the tiled kernel with a second output, the stage's ticks (k_bonds_tiled_tw) or its map words (k_bonds_tiled_maps)
int launch_tiled_out(gorder_hip_handle *h, const SubRange &s, const ExtraArgs &e) {
    const gorder::OrderRoute &route = s.route;
    const uint32_t nt = (uint32_t)h->plan.tiles.size();
    const gorder::FrameChunks c = gorder::extras_chunks(s.nf(), nt, h->sw.wg_target, h->wg_capacity, route.map_accumulate,
                                                        route.family == gorder::BondFamily::TiledTw);
    FrameArgs b = s.frames(c);
    const dim3 g(nt * c.n_chunks), blk(kBlock);
    const Item *items = bond_items(h, route);
    TIMING_MARK(h, route.label);
    with_npf(route.npf, [&](auto NPF) { with_bool(b.pbc, [&](auto PBC) { with_bool(b.leaflets, [&](auto LF) { with_axis(h->axis, [&](auto AX) {
        if (route.family == gorder::BondFamily::TiledMaps)
            hipLaunchKernelGGL((k_bonds_tiled_maps<NPF(), PBC(), LF(), AX()>), g, blk, h->lds_bytes, h->stream, b, e, b.xyz,
                               b.box9, b.aflags, b.arow, h->d_tiles, items, h->d_tile_slots, nt, h->lw);
        else with_bool(route.tw_maps, [&](auto MAPS) { with_bool(route.mom, [&](auto MOM) {
            if constexpr (!MOM() || (LF() && !MAPS()))
                hipLaunchKernelGGL((k_bonds_tiled_tw<NPF(), PBC(), LF(), AX(), MAPS(), MOM()>), g, blk, h->lds_bytes, h->stream, b, e,
                                   b.xyz, b.box9, b.aflags, b.arow, h->d_tiles, items, h->d_tile_slots, nt, h->lw);
        }); });
    }); }); }); });
    return GORDER_OK;
}

// second step of a staged pass: slot-major accumulation of the sub-range's staged samples in LDS (`per_item` samples an item)
int launch_map_accumulate(gorder_hip_handle *h, const SubRange &s, uint32_t rec_stride, const gorder::MapRun *runs,
                          const uint32_t *run_begin, uint32_t per_item) {
    const uint32_t n_acc = h->plan.n_acc;
    const uint32_t planes = h->tables.leaflets.method != GORDER_LEAFLETS_NONE ? 2u : 1u;
    const uint32_t ntm = h->map_nx * h->map_ny, n_words = planes * ntm;
    const gorder::FrameChunks m = gorder::map_chunks(s.nf(), n_acc, h->sw.map_chunks);       // (GORDER_HIP_MAP_CHUNKS)
    TIMING_MARK(h, "k_map_accumulate");
    hipLaunchKernelGGL(k_map_accumulate, dim3(n_acc * m.n_chunks), dim3(1024), n_words * sizeof(unsigned long long), h->stream,
                       h->d_map_rec, runs, run_begin, n_acc, s.nf(), rec_stride, m.frames_per_chunk, per_item, n_words, ntm,
                       h->d_map_packed, n_acc);
    return GORDER_OK;
}

// the bond tiles of a sub-range, by family
int launch_bond_pass(gorder_hip_handle *h, const SubRange &s, ExtraArgs &e) {
    using gorder::BondFamily;
    e.item_run = h->d_item_run;      // (k_bonds_tiled_tw only)
    switch (s.route.family) {
    case BondFamily::Classes: ST_TRY(launch_classes(h, s)); break;
    case BondFamily::Shells: ST_TRY(launch_shells(h, s, e)); break;
    case BondFamily::Dist: ST_TRY(launch_dist(h, s, e)); break;
    case BondFamily::Extras: ST_TRY(launch_extras(h, s, e)); break;
    default: ST_TRY(launch_tiled_out(h, s, e)); break;
    }
    if (s.route.map_accumulate) ST_TRY(launch_map_accumulate(h, s, e.rec_stride, h->d_runs, h->d_run_begin, 1u));
    HIP_TRY(h, hipGetLastError());
    return GORDER_OK;
}

// the order histogram over the united-atom tiles (GORDER_FLAG_UA_SAMPLES): k_bonds_dist's replicas, k_ua_extras' grid
int launch_ua_dist(gorder_hip_handle *h, const SubRange &s, const ExtraArgs &e) {
    const uint32_t nt = (uint32_t)h->plan.ua_tiles.size();
    const gorder::FrameChunks c = gorder::dist_chunks(s.nf(), nt, h->sw.wg_target, h->wg_capacity, h->hist_direct ? 0u : (uint32_t)h->hist_table_words,
                                                      h->sw.dist_samples_per_word, kDistChunkMax);
    FrameArgs b = s.frames(c);
    DistArgs da{};
    da.n_edges = h->hist_edges; da.edges = h->d_hist_edges; da.rep = h->hist.rep; da.n_rep = h->hist.n_rep;
    // the edges, then the table of the widest tile or the epilogue's sums, whichever is larger
    const size_t lds = kDistEdgeBytes + std::max<size_t>(kUaSumBytes, h->hist_direct ? 0u : h->hist_table_words * sizeof(uint32_t));
    const dim3 g((uint32_t)ua_grid(nt, c.n_chunks)), blk(kBlock);
    TIMING_MARK(h, "k_ua_dist");
    with_bool(literal_cosine(h), [&](auto AC) { with_bool(h->hist_direct, [&](auto DIRECT) {
        hipLaunchKernelGGL((k_ua_dist<AC(), DIRECT()>), g, blk, lds, h->stream, b, e, da, b.xyz, b.box9, b.aflags, b.arow, h->d_ua_tiles,
                           h->d_ua_items, h->d_ua_tile_slots, nt);
    }); });
    HIP_TRY(h, hipGetLastError());
    return GORDER_OK;
}

// ... and its united-atom tiles
int launch_ua_pass(gorder_hip_handle *h, const SubRange &s, ExtraArgs &e) {
    const gorder::OrderRoute &route = s.route;
    if (route.ua_kernel == gorder::UaKernel::Dist) return launch_ua_dist(h, s, e);
    const uint32_t nt = (uint32_t)h->plan.ua_tiles.size();
    const gorder::FrameChunks c = gorder::extras_chunks(s.nf(), nt, h->sw.wg_target, h->wg_capacity, route.map_accumulate, false);
    FrameArgs b = s.frames(c);
    e.item_run = h->d_ua_item_run;
    const dim3 g((uint32_t)ua_grid(nt, c.n_chunks)), blk(kBlock);
    TIMING_MARK(h, "k_ua_extras");
    with_bool(literal_cosine(h), [&](auto AC) { with_bool(route.ua_fast, [&](auto FAST) { with_int<0, 1, 2, 3>(route.ua_mode, [&](auto MODE) {
        if constexpr (FAST() && !AC())
            hipLaunchKernelGGL((k_ua_extras_fast<MODE()>), g, blk, 0, h->stream, b, e, b.xyz, b.box9, b.aflags, b.arow,
                               h->d_ua_tiles, h->d_ua_items, h->d_ua_tile_slots, nt, (const float *)e.inv_box);
        else if constexpr (!FAST())
            hipLaunchKernelGGL((k_ua_extras<AC(), MODE()>), g, blk, 0, h->stream, b, e, b.xyz, b.box9, b.aflags, b.arow,
                               h->d_ua_tiles, h->d_ua_items, h->d_ua_tile_slots, nt, (const float *)nullptr);
    }); }); });
    if (route.map_accumulate) ST_TRY(launch_map_accumulate(h, s, e.rec_stride, h->d_ua_runs, h->d_ua_run_begin, 3u));
    HIP_TRY(h, hipGetLastError());
    return GORDER_OK;
}

// Everything that scatters (route.extras, or united atoms): the bond tiles, then the united-atom tiles, a sub-range of the
// batch's frames at a time — as many as the packed map words, the staging block or the class rows hold
int launch_scatter_passes(gorder_hip_handle *h, const FrameArgs &a, const gorder::OrderRoute &route) {
    const Plan &p = h->plan;
    ExtraArgs e = h->extra;
    e.tw_sums = h->d_tw_sums; e.tw_cnts = h->d_tw_cnts; e.tw_row0 = h->n_frames;
    e.shapes = h->d_shapes; e.inv_box = nullptr;
    if (route.ua_fast && a.pbc) {      // 1 / box edge per frame, once per frame instead of once per lane and frame
        ST_TRY(ensure(h, h->d_inv_box, (size_t)a.n_frames * 8));
        hipLaunchKernelGGL(k_inv_box, dim3((4u * a.n_frames + 255u) / 256u), dim3(256), 0, h->stream, a.box9, a.n_frames, h->d_inv_box);
        e.inv_box = h->d_inv_box;
    }
    e.dyn = (h->dyn || h->manual_active) ? h->d_dyn_normals : nullptr;
    const bool staged = route.map_accumulate;
    const size_t rec_per_frame = std::max(p.ua_tiles.size() * 3u, route.extras ? p.tiles.size() : (size_t)0) * kBlock;   // staged words per frame
    const long forced_limit = h->sw.map_fold_limit;    // GORDER_HIP_MAP_FOLD_LIMIT lowers the limit (tests)
    const uint64_t fold_limit = forced_limit >= 2 && (unsigned long long)forced_limit <= kMapFoldLimit ? (uint64_t)forced_limit : kMapFoldLimit;
    uint32_t sub = gorder::map_subrange(a.n_frames, e.maps != 0, staged, fold_limit, h->map_max_mol, rec_per_frame);
    // neighbour classes: the class rows hold the whole batch where it fits them (gorder_hip_neighbour_class_rows then returns
    // it), else one sub-range at a time
    bool class_rows_whole = false;
    if (route.family == gorder::BondFamily::Classes) {
        class_rows_whole = gorder::class_rows_whole(a.n_frames, p.n_mol_total, h->sw.nb_row_bytes);
        sub = gorder::class_subrange(a.n_frames, p.n_mol_total, h->sw.nb_subrange, h->sw.nb_row_bytes);     // (GORDER_HIP_NB_SUBRANGE, GORDER_HIP_NB_ROW_BYTES)
        ST_TRY(ensure(h, h->nb.rows, (size_t)(class_rows_whole ? a.n_frames : sub) * p.n_mol_total));
    }
    if (staged) ST_TRY(ensure(h, h->d_map_rec, rec_per_frame * (((size_t)sub + 15) / 16 * 16)));
    e.map_rec = staged ? h->d_map_rec : nullptr;
    for (uint32_t lo = 0; lo < a.n_frames; lo += sub) {
        const SubRange s{a, route, lo, std::min(a.n_frames, lo + sub), class_rows_whole};
        if (e.maps) {
            const uint64_t cost = (uint64_t)s.nf() * h->map_max_mol;
            if (h->map_pending + cost >= fold_limit) ST_TRY(fold_maps(h));
            h->map_pending += cost;
        }
        e.rec_frame0 = lo; e.rec_stride = (s.nf() + 15u) / 16u * 16u;
        if (route.extras && !p.tiles.empty()) ST_TRY(launch_bond_pass(h, s, e));
        if (!p.ua_tiles.empty() && route.ua_kernel != gorder::UaKernel::Mol) ST_TRY(launch_ua_pass(h, s, e));
    }
    return GORDER_OK;
}

int launch_bonds_direct(gorder_hip_handle *h, const FrameArgs &a) {
    const uint32_t n_items = (uint32_t)h->plan.direct.size(), bpc = (n_items + kBlock - 1) / kBlock;
    const gorder::FrameChunks c = gorder::direct_chunks(a.n_frames, bpc, h->sw.wg_target);
    FrameArgs b = a;
    b.frames_per_chunk = c.frames_per_chunk;
    TIMING_MARK(h, "k_bonds_direct");
    with_bool(literal_cosine(h), [&](auto AC) { hipLaunchKernelGGL(k_bonds_direct<AC()>, dim3(bpc * c.n_chunks), dim3(kBlock), 0, h->stream, b, h->d_direct, n_items, bpc); });
    HIP_TRY(h, hipGetLastError());
    return GORDER_OK;
}

int launch_orders(gorder_hip_handle *h, FrameArgs &a, const gorder::OrderRoute &route) {
    using gorder::BondFamily;
    if (h->dyn && !h->manual_active) ST_TRY(run_dynamic_normals(h, a));
    if (h->extra.geom_kind) ST_TRY(launch_geometry_shapes(h, a));
    if (route.family == BondFamily::Tiled || route.family == BondFamily::Gather) ST_TRY(launch_tiled(h, a, route));
    const bool ua_mol = route.ua_kernel == gorder::UaKernel::Mol;      // (k_ua_mol is the united-atom pass of such a handle)
    if (route.family == BondFamily::TiledMol || ua_mol) ST_TRY(launch_molecule_rows(h, a, route));
    if (route.extras || (route.ua_mode >= 0 && !ua_mol)) ST_TRY(launch_scatter_passes(h, a, route));
    if (route.direct) ST_TRY(launch_bonds_direct(h, a));
    return GORDER_OK;       // (the frames are counted by k_batch_end, which also closes the batch's timing chain)
}

// ---- collected history (gorder_hip_set_collect): staging block -> pinned chunks ----------------------------------------
// reserve `n_rows` rows labelled `frames` and queue the copies that fill them from the staging block (a batch that crosses
// a chunk boundary takes more than one copy); nothing waits
int collect_copy_out(gorder_hip_handle *h, gorder::CollectStore &store, const void *d_block, const uint64_t *frames, size_t n_rows) {
    std::vector<gorder::CollectPiece> pieces;
    if (!store.reserve(frames, n_rows, pieces)) return fail(h, GORDER_ERR_DEVICE, "collect: no pinned host memory for the history");
    const char *src = static_cast<const char *>(d_block);
    for (const gorder::CollectPiece &pc : pieces) {
        const size_t bytes = pc.rows * store.row_bytes();
        HIP_TRY(h, hipMemcpyAsync(pc.host, src, bytes, hipMemcpyDeviceToHost, h->stream));
        src += bytes;
    }
    return GORDER_OK;
}

// rows first_row .. of d_aflags are the sides of the assignment frames `frames`: pack and keep them
int collect_flag_rows(gorder_hip_handle *h, size_t first_row, const std::vector<uint64_t> &frames) {
    if (frames.empty()) return GORDER_OK;
    const uint32_t n_mol = h->plan.n_mol_total, wpr = (uint32_t)gorder::collect_flag_words(n_mol);
    const unsigned long long total = (unsigned long long)frames.size() * wpr;
    if ((total + 3u) / 4u > 0x7fffffffull || frames.size() > 0xffffffffull) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "collect: batch too large");
    int st;
    if ((st = ensure(h, h->d_collect_words, (size_t)total)) != GORDER_OK) return st;
    TIMING_MARK(h, "k_collect_flags");
    hipLaunchKernelGGL(k_collect_flags, dim3((uint32_t)((total + 3u) / 4u)), dim3(256), 0, h->stream,
                       h->d_aflags + first_row * (size_t)n_mol, n_mol, (uint32_t)frames.size(), wpr, h->d_collect_words);
    HIP_TRY(h, hipGetLastError());
    return collect_copy_out(h, h->collect_flags, h->d_collect_words, frames.data(), frames.size());
}

// the batch's d_dyn_normals [n_frames][n_mol_total] as rows of three floats a molecule
int collect_normal_rows(gorder_hip_handle *h, const uint64_t *frame_index, uint32_t n_frames, const uint8_t *touched) {
    const unsigned long long n = (unsigned long long)n_frames * h->plan.n_mol_total;
    if ((n + 255u) / 256u > 0x7fffffffull) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "collect: batch too large");
    int st;
    if ((st = ensure(h, h->d_collect_vec, (size_t)n)) != GORDER_OK) return st;
    TIMING_MARK(h, "k_collect_normals");
    hipLaunchKernelGGL(k_collect_normals, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, h->stream,
                       (const float4 *)h->d_dyn_normals, touched, n, h->d_collect_vec);
    HIP_TRY(h, hipGetLastError());
    return collect_copy_out(h, h->collect_normals, h->d_collect_vec, frame_index, n_frames);
}

// ---- whole-trajectory manual tables: expand what a batch needs (kernels_replay.h) -----------------------------------------
// a small list of 32-bit rows for this batch, behind everything queued so far
int upload_rows(gorder_hip_handle *h, DBuf<uint32_t> &buf, const std::vector<uint32_t> &rows) {
    ST_TRY(ensure(h, buf, rows.size()));
    HIP_TRY(h, hipMemcpyAsync(buf, rows.data(), rows.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    return GORDER_OK;
}
// ... and one that batches repeat (d_arow, d_aframes): `held` is what the buffer holds while `valid`, and equal batches (same
// length, same assignment pattern) skip the copy
int upload_if_changed(gorder_hip_handle *h, DBuf<uint32_t> &buf, std::vector<uint32_t> &held, bool &valid, const std::vector<uint32_t> &rows) {
    bool grew = false;
    const int st = ensure(h, buf, rows.size(), &grew);
    if (grew || st != GORDER_OK) valid = false;      // a new allocation holds nothing yet
    if (st != GORDER_OK || (valid && held == rows)) return st;
    ST_TRY(upload_rows(h, buf, rows));
    held = rows;
    valid = true;
    return GORDER_OK;
}

// rows 1.. of d_aflags from the table rows rb.expand
int replay_flag_rows(gorder_hip_handle *h, const gorder::ReplayLeafletBatch &rb) {
    if (rb.expand.empty()) return GORDER_OK;
    const uint32_t n_mol = h->plan.n_mol_total, wpr = (uint32_t)gorder::replay_flag_words(n_mol);
    const unsigned long long total = (unsigned long long)rb.expand.size() * wpr;
    if ((total + 3u) / 4u > 0x7fffffffull) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "manual leaflet table: batch too large");
    ST_TRY(upload_if_changed(h, h->d_aframes, h->up_aframes, h->up_aframes_valid, rb.expand));
    TIMING_MARK(h, "k_replay_flags");
    hipLaunchKernelGGL(k_replay_flags, dim3((uint32_t)((total + 3u) / 4u)), dim3(256), 0, h->stream, h->d_ltable, h->d_aframes,
                       (uint32_t)rb.expand.size(), wpr, n_mol, h->tables.leaflets.flip ? 1u : 0u, h->d_aflags + n_mol);
    HIP_TRY(h, hipGetLastError());
    return GORDER_OK;
}

// d_dyn_normals [n_frames][n_mol_total] from the table rows row_of_frame
int replay_normal_rows(gorder_hip_handle *h, const std::vector<uint32_t> &row_of_frame) {
    const uint32_t n_mol = h->plan.n_mol_total;
    const unsigned long long n = (unsigned long long)row_of_frame.size() * n_mol;
    if ((n + 255u) / 256u > 0x7fffffffull) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "manual normal table: batch too large");
    int st;
    if ((st = ensure(h, h->d_dyn_normals, (size_t)n)) != GORDER_OK) return st;
    if ((st = upload_rows(h, h->d_nrow, row_of_frame)) != GORDER_OK) return st;
    if (!n) return GORDER_OK;
    TIMING_MARK(h, "k_replay_normals");
    hipLaunchKernelGGL(k_replay_normals, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, h->stream, h->d_ntable, h->d_nrow, n_mol, n,
                       h->d_dyn_normals);
    HIP_TRY(h, hipGetLastError());
    return GORDER_OK;
}

}  // namespace

// ---- RCCL: SystemTopology::reduce across the GPUs of a node (topology/mod.rs:256-272) -----------------------------
// The library does not link RCCL: the few entry points are bound at the first call (dlopen by SONAME, so a process
// that already holds RCCL — e.g. through PyTorch — shares that copy; otherwise /opt/rocm's).
namespace {
struct UniqueId { char internal[128]; };     // ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES = 128)
struct RcclApi {
    void *lib = nullptr;
    int (*get_unique_id)(void *) = nullptr;
    int (*comm_init_rank)(void **, int, UniqueId /* ncclUniqueId, by value */, int) = nullptr;
    int (*comm_destroy)(void *) = nullptr;
    int (*all_reduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*group_start)() = nullptr;
    int (*group_end)() = nullptr;
    const char *(*get_error_string)(int) = nullptr;
};
constexpr int kNcclInt64 = 4, kNcclSum = 0;   // ncclDataType_t / ncclRedOp_t values of rccl.h
RcclApi *rccl_api(std::string *why) {
    static RcclApi api;
    static std::once_flag once;
    static std::string err;
    std::call_once(once, [&]() {
        const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        for (const char *n : names)
            if ((api.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) break;
        if (!api.lib) {
            err = std::string("cannot load RCCL: ") + dlerror();
        } else {
            api.get_unique_id = (decltype(api.get_unique_id))dlsym(api.lib, "ncclGetUniqueId");
            api.comm_init_rank = (decltype(api.comm_init_rank))dlsym(api.lib, "ncclCommInitRank");
            api.comm_destroy = (decltype(api.comm_destroy))dlsym(api.lib, "ncclCommDestroy");
            api.all_reduce = (decltype(api.all_reduce))dlsym(api.lib, "ncclAllReduce");
            api.group_start = (decltype(api.group_start))dlsym(api.lib, "ncclGroupStart");
            api.group_end = (decltype(api.group_end))dlsym(api.lib, "ncclGroupEnd");
            api.get_error_string = (decltype(api.get_error_string))dlsym(api.lib, "ncclGetErrorString");
            if (!api.get_unique_id || !api.comm_init_rank || !api.comm_destroy || !api.all_reduce || !api.group_start ||
                !api.group_end) {
                err = "RCCL library lacks an expected entry point";
                api.lib = nullptr;
            }
        }
    });
    if (!api.lib) { if (why) *why = err; return nullptr; }
    return &api;
}
std::string rccl_error(const RcclApi *api, const char *what, int rc) {
    return std::string(what) + ": " + (api->get_error_string ? api->get_error_string(rc) : "RCCL error") + " (" + std::to_string(rc) + ")";
}
}  // namespace


extern "C" {

const char *gorder_hip_strerror(int status) {
    switch (status) {
        case GORDER_OK: return "ok";
        case GORDER_ERR_UNDEFINED_BOX: return "system has undefined simulation box";
        case GORDER_ERR_NOT_ORTHOGONAL_BOX: return "the simulation box is not orthogonal";
        case GORDER_ERR_ZERO_BOX: return "all dimensions of the simulation box are zero";
        case GORDER_ERR_UNDEFINED_POSITION: return "atom has an undefined position";
        case GORDER_ERR_INVALID_GLOBAL_MEMBRANE_CENTER: return "could not calculate global membrane center";
        case GORDER_ERR_INVALID_LOCAL_MEMBRANE_CENTER: return "could not calculate local membrane center";
        case GORDER_ERR_DYNAMIC_NORMAL: return "not enough points for dynamic local membrane normal calculation (need 3)";
        case GORDER_ERR_MANUAL_LEAFLET_FRAME: return "manual leaflet assignment: no row for the frame";
        case GORDER_ERR_MANUAL_NORMAL_FRAME: return "manual membrane normals: no row for the frame";
        case GORDER_ERR_INVALID_ARGUMENT: return "invalid argument";
        case GORDER_ERR_DEVICE: return "HIP runtime error";
        case GORDER_ERR_NO_DEVICE: return "no HIP device available (this library has no CPU fallback)";
        case GORDER_ERR_BOX_RANGE: return "box edge <= 0 or coordinate too far outside the box";
        case GORDER_ERR_LEAFLETS_NOT_PRIMED: return "leaflet assignment missing for the first frame";
        case GORDER_ERR_OVERFLOW: return "order accumulator overflowed";
        case GORDER_ERR_TRAJECTORY_FORMAT: return "corrupt or truncated trajectory frame";
        case GORDER_ERR_CLUSTERING: return "clustering: a distance between head atoms or to their centre is not finite";
        case GORDER_ERR_CLUSTER_MATCH: return "clustering: the clusters match neither leaflet of the previous assignment frame (80 % overlap)";
        default: return "unknown status";
    }
}

namespace {
__global__ void k_selftest_arithmetic(uint64_t n, uint64_t seed, unsigned long long *mismatches) {
    uint64_t bad_div = 0, bad_sqrt = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t x = (i + 1) * 0x9E3779B97F4A7C15ull + seed;          // splitmix64
        auto next = [&]() {
            x += 0x9E3779B97F4A7C15ull;
            uint64_t z = x;
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            return z ^ (z >> 31);
        };
        auto make = [&](int e_lo, int e_hi, bool sign) {                // random mantissa, exponent uniform in [e_lo, e_hi]
            const uint64_t r = next();
            const uint32_t e = (uint32_t)(127 + e_lo + (int)((r >> 32) % (uint64_t)(e_hi - e_lo + 1)));
            uint32_t bits = (e << 23) | (uint32_t)(r & 0x7fffffu);
            if (sign && (r >> 63)) bits |= 0x80000000u;
            return __uint_as_float(bits);
        };
        float d = make(-40, 39, false);
        if (i % 1024u == 0) d = 0x1p+40f;
        if (i % 1024u == 1) d = 0x1p-40f;
        float num = make(-100, 60, true);
        if (i % 64u == 0) num = 0.0f;
        if (i % 64u == 1) num = d;                                        // quotient exactly 1
        if (i % 64u == 2) num = d * 0.5f;                                 // exact ties of the rounding to a tile index
        const float q_core = gm_div_core(num, d), q_ieee = num / d;
        if (__float_as_uint(q_core) != __float_as_uint(q_ieee)) bad_div++;
        const float s_core = gm_sqrt_core(d), s_ieee = __builtin_sqrtf(d);
        if (__float_as_uint(s_core) != __float_as_uint(s_ieee)) bad_sqrt++;
        // acos with the cores inside against acos with the IEEE operations: arguments over the whole of [-1, 1]
        // (every exponent down to 2^-60, both ends, the ties of the range split)
        float xa = make(-60, -1, true);
        if (i % 16u == 0) xa = __builtin_copysignf(1.0f - __uint_as_float(0x33800000u) * (float)(next() & 0xffffu), xa);   // 1 - k 2^-24
        if (i % 4096u == 1) xa = 1.0f;
        if (i % 4096u == 2) xa = -1.0f;
        if (i % 4096u == 3) xa = 0.5f;
        if (i % 4096u == 4) xa = 0.0f;
        if (__float_as_uint(gm_acosf_t<true>(xa)) != __float_as_uint(gm_acosf_t<false>(xa))) bad_sqrt++;
    }
    if (bad_div) atomicAdd(&mismatches[0], (unsigned long long)bad_div);
    if (bad_sqrt) atomicAdd(&mismatches[1], (unsigned long long)bad_sqrt);
}
}  // namespace

int gorder_hip_selftest_arithmetic(int device, uint64_t n, uint64_t seed, uint64_t mismatches[2]) {
    if (!mismatches) return GORDER_ERR_INVALID_ARGUMENT;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return GORDER_ERR_NO_DEVICE;
    if (device < 0 || device >= count || hipSetDevice(device) != hipSuccess) return GORDER_ERR_INVALID_ARGUMENT;
    DBuf<u64> d;
    if (!d.alloc(2)) return GORDER_ERR_DEVICE;
    int st = GORDER_OK;
    if (hipMemset(d, 0, 2 * sizeof(unsigned long long)) != hipSuccess) st = GORDER_ERR_DEVICE;
    if (st == GORDER_OK) {
        hipLaunchKernelGGL(k_selftest_arithmetic, dim3(4096), dim3(256), 0, 0, n, seed, d.get());
        unsigned long long out[2] = {0, 0};
        if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(out, d, sizeof(out), hipMemcpyDeviceToHost) != hipSuccess)
            st = GORDER_ERR_DEVICE;
        mismatches[0] = out[0];
        mismatches[1] = out[1];
    }
    return st;
}

namespace {
__global__ void k_selftest_trig(int fn, uint32_t first_bits, uint32_t stride, uint32_t n, float *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = __uint_as_float(first_bits + i * stride);
    float s, c;
    gm_sincosf_0pi(x, s, c);
    out[i] = fn == 0 ? gm_acosf_t<false>(x) : fn == 1 ? gm_acosf_t<true>(x) : fn == 2 ? c : s;
}
}  // namespace

int gorder_hip_selftest_trig(int device, int fn, uint32_t first_bits, uint32_t stride, uint32_t n, float *out) {
    if (!out || fn < 0 || fn > 3) return GORDER_ERR_INVALID_ARGUMENT;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return GORDER_ERR_NO_DEVICE;
    if (device < 0 || device >= count || hipSetDevice(device) != hipSuccess) return GORDER_ERR_INVALID_ARGUMENT;
    if (n == 0) return GORDER_OK;
    DBuf<float> d;
    if (!d.alloc(n)) return GORDER_ERR_DEVICE;
    hipLaunchKernelGGL(k_selftest_trig, dim3((n + 255u) / 256u), dim3(256), 0, 0, fn, first_bits, stride, n, d.get());
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(out, d, (size_t)n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
        return GORDER_ERR_DEVICE;
    return GORDER_OK;
}

namespace {
// every primitive of wave_ops.h on one value per thread; row r of an output = what every lane holds behind primitive r
// (the order of the rows: gorder_hip.h)
__global__ __launch_bounds__(1024) void k_selftest_wave_ops(const double *in_f64, const float *in_f32, const uint32_t *in_u32,
                                                            int finfo_empty, double *out_f64, float *out_f32, uint32_t *out_u32,
                                                            uint4 *out_finfo) {
    __shared__ double scratch[32];
    __shared__ float fscratch[32], l_lo[16], l_hi[16];
    __shared__ uint32_t l_flags[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, n = blockDim.x;
    const double d = in_f64[tid];
    const float x = in_f32[tid];
    const uint32_t u = in_u32[tid];
    if (tid < 16u) { l_lo[tid] = 3.0e38f; l_hi[tid] = -3.0e38f; l_flags[tid] = 0u; }   // (the waves that are not here)
    __syncthreads();
    double s = d, q = 3.0 * d, bs[2] = {d, 3.0 * d};
    float lo4 = x, hi4 = x, lo2 = x, hi2 = x, lo3 = x, hi3 = x, blo = x, bhi = x;
    uint32_t or3 = u;
    wave_sum2_minmax_bfly(s, q, lo4, hi4);
    wave_minmax_bfly(lo2, hi2);
    wave_minmax_or_bfly(lo3, hi3, or3);
    block_sum_n<2>(bs, scratch);
    block_minmax(blo, bhi, fscratch);
    const double o64[GORDER_WAVE_OPS_F64_ROWS] = {row_sum(d), rows_to_wave(row_sum(d)), wave_sum_rows(d), wave_scan_rows(d, lane),
                                                  wave_sum_bfly(d), bs[0], bs[1], lane_value(d, 47), s, q};
    const float o32[GORDER_WAVE_OPS_F32_ROWS] = {row_sum(x), rows_to_wave(row_sum(x)), wave_sum_rows(x), wave_min_rows(x),
                                                 wave_max_rows(x), lo2, hi2, blo, bhi, dpp_or_self<0x111>(x),
                                                 dpp_or_zero<0x143, 0xc>(x), lane_value(x, 47), lo4, hi4, lo3, hi3};
    const uint32_t ou[GORDER_WAVE_OPS_U32_ROWS] = {row_sum(u), rows_to_wave(row_sum(u)), wave_sum_rows(u), wave_scan_rows(u, lane),
                                                   wave_scan_shfl(u, lane), or3, wave_max_bfly(u),
                                                   (uint32_t)wave_sum_rows((int)u), lane_value(u, 47)};
    for (int r = 0; r < GORDER_WAVE_OPS_F64_ROWS; r++) out_f64[r * n + tid] = o64[r];
    for (int r = 0; r < GORDER_WAVE_OPS_F32_ROWS; r++) out_f32[r * n + tid] = o32[r];
    for (int r = 0; r < GORDER_WAVE_OPS_U32_ROWS; r++) out_u32[r * n + tid] = ou[r];
    // the finfo record twice: every flag kept, and bit 0 only; word 8 = the flags thread 0 leaves the fold with
    const float zlo = finfo_empty ? 3.0e38f : x, zhi = finfo_empty ? -3.0e38f : x;
    uint32_t fl = u;
    block_finfo_record(zlo, zhi, fl, ~0u, l_lo, l_hi, l_flags, out_finfo);
    if (tid == 0u) out_finfo[2].x = fl;
    __syncthreads();
    fl = u;
    block_finfo_record(zlo, zhi, fl, 1u, l_lo, l_hi, l_flags, out_finfo + 1);
}
}  // namespace

int gorder_hip_selftest_wave_ops(int device, uint32_t block, const double *f64, const float *f32, const uint32_t *u32,
                                 int finfo_empty, double *out_f64, float *out_f32, uint32_t *out_u32, uint32_t *out_finfo) {
    if (!f64 || !f32 || !u32 || !out_f64 || !out_f32 || !out_u32 || !out_finfo || block < 64u || block > 1024u || (block & 63u))
        return GORDER_ERR_INVALID_ARGUMENT;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return GORDER_ERR_NO_DEVICE;
    if (device < 0 || device >= count || hipSetDevice(device) != hipSuccess) return GORDER_ERR_INVALID_ARGUMENT;
    // one allocation: the inputs, then the outputs, the widest type first (everything stays aligned)
    const size_t n = block, b_fi = 0, b_i64 = 48, b_o64 = b_i64 + 8 * n, b_i32 = b_o64 + 8 * n * GORDER_WAVE_OPS_F64_ROWS,
                 b_iu = b_i32 + 4 * n, b_o32 = b_iu + 4 * n, b_ou = b_o32 + 4 * n * GORDER_WAVE_OPS_F32_ROWS,
                 bytes = b_ou + 4 * n * GORDER_WAVE_OPS_U32_ROWS;
    DBuf<char> owned;
    if (!owned.alloc(bytes)) return GORDER_ERR_DEVICE;
    char *d = owned;
    int st = GORDER_OK;
    if (hipMemset(d, 0, bytes) != hipSuccess || hipMemcpy(d + b_i64, f64, 8 * n, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d + b_i32, f32, 4 * n, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d + b_iu, u32, 4 * n, hipMemcpyHostToDevice) != hipSuccess)
        st = GORDER_ERR_DEVICE;
    if (st == GORDER_OK) {
        hipLaunchKernelGGL(k_selftest_wave_ops, dim3(1), dim3(block), 0, 0, (const double *)(d + b_i64), (const float *)(d + b_i32),
                           (const uint32_t *)(d + b_iu), finfo_empty, (double *)(d + b_o64), (float *)(d + b_o32),
                           (uint32_t *)(d + b_ou), (uint4 *)(d + b_fi));
        if (hipDeviceSynchronize() != hipSuccess ||
            hipMemcpy(out_f64, d + b_o64, 8 * n * GORDER_WAVE_OPS_F64_ROWS, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(out_f32, d + b_o32, 4 * n * GORDER_WAVE_OPS_F32_ROWS, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(out_u32, d + b_ou, 4 * n * GORDER_WAVE_OPS_U32_ROWS, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(out_finfo, d + b_fi, 4 * GORDER_WAVE_OPS_FINFO_WORDS, hipMemcpyDeviceToHost) != hipSuccess)
            st = GORDER_ERR_DEVICE;
    }
    return st;
}

int gorder_hip_plan_tables(const gorder_tables_t *tables, gorder_hip_plan_t *out, int *selfcheck) {
    if (!tables || !out) return GORDER_ERR_INVALID_ARGUMENT;
    Plan p;
    ST_TRY(gorder::build_plan(*tables, gorder::read_switches(::getenv).force_direct, p));     // (GORDER_HIP_FORCE_DIRECT, as at create)
    out->n_tiles = (uint32_t)p.tiles.size();
    out->block_threads = kBlock;
    out->max_window_atoms = p.max_window;
    out->n_direct_items = (uint32_t)p.direct.size();
    out->frames_per_stage = kFramesPerStage;
    const uint32_t lw = ((3u * p.max_window + 3u + 3u) / 4u) * 4u;
    size_t lds = (size_t)kFramesPerStage * lw * sizeof(float);
    if (lds < (size_t)kBlock * 24) lds = (size_t)kBlock * 24;
    out->lds_bytes = (uint32_t)lds;
    out->map_staged = 0;         // decided at gorder_hip_create (device LDS size, GORDER_HIP_MAP_DIRECT)
    out->map_lds_bytes = 0;
    out->leaflets_one_read = p.spec_ok ? 1u : 0u;
    if (selfcheck) *selfcheck = gorder::selfcheck_plan(*tables, p);
    return GORDER_OK;
}

static size_t cl_frame_bytes(uint32_t n, uint32_t m_max);
static size_t clcut_frame_bytes(uint32_t n, uint32_t m_max);

// ---- gorder_hip_create, feature by feature: each validates, builds and allocates what its own feature needs ------------------
static int create_ordermaps(gorder_hip_handle *h, const gorder_tables_t *t) {
    const gorder_ordermap_t &om = t->ordermap;
    if (!om.enabled) return GORDER_OK;
    const Plan &p = h->plan;
    ExtraArgs &e = h->extra;
    if (!(om.bin[0] > 0.0f) || !(om.bin[1] > 0.0f) || om.plane > 2)
        return fail(h, GORDER_ERR_INVALID_ARGUMENT, "ordermap bin/plane");
    // groan_rs GridMap::new: n = round(span / bin) + 1 tiles per axis
    const float fx = roundf((om.span_x[1] - om.span_x[0]) / om.bin[0]);
    const float fy = roundf((om.span_y[1] - om.span_y[0]) / om.bin[1]);
    if (!(fx >= 0.0f) || !(fy >= 0.0f) || fx > 65535.0f || fy > 65535.0f)
        return fail(h, GORDER_ERR_INVALID_ARGUMENT, "ordermap span");
    h->map_nx = (uint32_t)fx + 1u;
    h->map_ny = (uint32_t)fy + 1u;
    const size_t nmap = 3 * (size_t)p.n_acc * h->map_nx * h->map_ny;
    const size_t npk = (t->leaflets.method != GORDER_LEAFLETS_NONE ? 2 : 1) * (nmap / 3);
    ST_TRY(allocate(h, h->d_map_sums, nmap, 0));
    ST_TRY(allocate(h, h->d_map_cnts, nmap, 0));
    ST_TRY(allocate(h, h->d_map_packed, npk, 0));
    // united atoms: stage + accumulate in LDS when one slot's packed map (x2 with leaflets) fits
    const size_t lds_bytes = npk / p.n_acc * sizeof(u64);
    h->map_lds_bytes = lds_bytes;
    if (lds_bytes <= 150u * 1024u && !h->sw.map_direct) {      // (GORDER_HIP_MAP_DIRECT)
        ST_TRY(upload(h, h->d_ua_runs, p.ua_runs));
        ST_TRY(upload(h, h->d_ua_run_begin, p.ua_run_begin));
        ST_TRY(upload(h, h->d_runs, p.runs));
        ST_TRY(upload(h, h->d_run_begin, p.run_begin));
        ST_TRY(upload(h, h->d_items_by_slot, p.items_by_slot));
        ST_TRY(upload(h, h->d_ua_item_run, p.ua_item_run));
        HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void *>(k_map_accumulate),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
        h->map_staged = true;
    }
    e.maps = 1; e.plane = om.plane; e.x0 = om.span_x[0]; e.y0 = om.span_y[0];
    e.binx = om.bin[0]; e.biny = om.bin[1]; e.nx = h->map_nx; e.ny = h->map_ny;
    e.inv_binx = 1.0f / om.bin[0]; e.inv_biny = 1.0f / om.bin[1];
    e.bin_core = (om.bin[0] >= 0x1p-40f && om.bin[0] <= 0x1p+40f && om.bin[1] >= 0x1p-40f && om.bin[1] <= 0x1p+40f) ? 1 : 0;
    e.map_packed = h->d_map_packed;
    return GORDER_OK;
}

static int create_geometry(gorder_hip_handle *h, const gorder_tables_t *t) {
    const gorder_geometry_t &ge = t->geometry;
    if (ge.kind == GORDER_GEOM_NONE) return GORDER_OK;
    ExtraArgs &e = h->extra;
    if (ge.kind > GORDER_GEOM_SPHERE || ge.reference > GORDER_GEOMREF_GROUP || ge.orientation > 2)
        return fail(h, GORDER_ERR_INVALID_ARGUMENT, "geometry kind/reference/orientation");
    if (ge.reference == GORDER_GEOMREF_BOX_CENTER && !t->handle_pbc)
        return fail(h, GORDER_ERR_INVALID_ARGUMENT, "box-centre reference needs handle_pbc (pbc.rs:243-245)");
    if (ge.reference == GORDER_GEOMREF_POINT && t->handle_pbc &&
        !(ge.structure_box[0] > 0.0f && ge.structure_box[1] > 0.0f && ge.structure_box[2] > 0.0f))
        return fail(h, GORDER_ERR_INVALID_ARGUMENT, "geometry.structure_box");
    if (ge.reference == GORDER_GEOMREF_GROUP) {
        if (!ge.group || ge.n_group == 0) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "geometry.group");
        std::vector<uint32_t> grp(ge.group, ge.group + ge.n_group);
        for (uint32_t a : grp)
            if (a >= t->n_atoms) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "geometry group index out of range");
        ST_TRY(upload(h, h->d_geom_group, grp));
    }
    e.geom_kind = (int)ge.kind; e.geom_invert = ge.invert ? 1 : 0; e.geom_orient = (int)ge.orientation;
    e.geom_thr = local_radius_threshold(ge.radius);
    h->tables.geometry.group = nullptr;
    return GORDER_OK;
}

// the error words, the accumulator block the handle owns and its replicas
static int create_accumulators(gorder_hip_handle *h) {
    const Plan &p = h->plan;
    ST_TRY(allocate(h, h->d_err, kErrWords + 2u));     // (+ the ticket of k_batch_end)
    HIP_TRY(h, hipMemset(h->d_err, 0xff, kErrWords * sizeof(uint32_t)));   // kErrNone
    HIP_TRY(h, hipMemset(h->d_err + kErrWords, 0, 2u * sizeof(uint32_t)));
    h->acc_words = 4 * (size_t)p.n_acc + 1;
    ST_TRY(allocate(h, h->own_acc, h->acc_words, 0));
    h->d_acc = h->own_acc;
    return p.n_acc ? allocate(h, h->d_rep, (size_t)h->sw.replicas * 4u * p.n_acc, 0) : GORDER_OK;
}

// k_local_build (dynamic normals, local leaflets) takes more dynamic LDS than a kernel gets unasked
static int local_build_attributes(gorder_hip_handle *h) {
    for (const void *fn : {reinterpret_cast<const void *>(k_local_build<2>), reinterpret_cast<const void *>(k_local_build<5>),
                           reinterpret_cast<const void *>(k_local_build<kLocalBuildTrips>)})
        HIP_TRY(h, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLocalBuildLds));
    return GORDER_OK;
}

static int create_dynamic_normals(gorder_hip_handle *h, const gorder_tables_t *t) {
    const gorder_dynamic_normal_t &dn = t->dynamic_normal;
    if (!dn.enabled) return GORDER_OK;
    const Plan &p = h->plan;
    if (!(dn.radius > 0.0f)) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "dynamic normals need a positive radius");
    if (!dn.cloud || dn.n_cloud == 0) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "dynamic normals need the NormalHeads group");
    if (!p.direct.empty()) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "dynamic normals: a bond spans more than the LDS window");
    std::vector<uint32_t> cloud(dn.cloud, dn.cloud + dn.n_cloud), nheads;
    for (uint32_t a : cloud)
        if (a >= t->n_atoms) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "NormalHeads index out of range");
    for (uint32_t m = 0; m < t->n_molecule_types; m++) {
        const gorder_moltype_t &mt = t->molecule_types[m];
        if (!mt.normal_heads) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "dynamic normals need normal_heads[] per molecule type");
        for (uint32_t k = 0; k < mt.n_molecules; k++) {
            if (mt.normal_heads[k] >= t->n_atoms) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "normal head index out of range");
            nheads.push_back(mt.normal_heads[k]);
        }
    }
    ST_TRY(upload(h, h->d_dyn_cloud, cloud));
    ST_TRY(upload(h, h->d_dyn_heads, nheads));
    h->host_dyn_heads = nheads;
    const size_t nm = dn.n_cloud, ncell = (size_t)kLocalMaxCells1D * kLocalMaxCells1D;
    const size_t sl = h->dyn_slab = local_slab_frames(nm, h->sw.local_slab);
    ST_TRY(local_build_attributes(h));
    ST_TRY(allocate(h, h->d_dyn_cell_of, sl * nm));
    ST_TRY(allocate(h, h->d_dyn_rec, sl * nm * 4));
    ST_TRY(allocate(h, h->d_dyn_count, sl * (2 * ncell + 1)));
    ST_TRY(allocate(h, h->d_dyn_cov, sl * (size_t)(p.n_mol_total ? p.n_mol_total : 1)));
    h->dyn = true;
    return GORDER_OK;
}

// what every leaflet method reads: each molecule's head (`heads`, kept for the methods below), the methyls of the individual
// method, the membrane group of the global and local ones
static int create_leaflet_tables(gorder_hip_handle *h, const gorder_tables_t *t, std::vector<uint32_t> &heads) {
    const gorder_leaflets_t &lf = t->leaflets;
    const Plan &p = h->plan;
    if (lf.method > GORDER_LEAFLETS_CLUSTERING) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "leaflets.method");
    if (lf.method != GORDER_LEAFLETS_SPHERICAL && lf.method != GORDER_LEAFLETS_CLUSTERING && lf.normal_dim > 2) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "leaflets.normal_dim");
    std::vector<uint32_t> mb(1, 0), ma;
    for (uint32_t m = 0; m < t->n_molecule_types; m++) {
        const gorder_moltype_t &mt = t->molecule_types[m];
        if (lf.method != GORDER_LEAFLETS_MANUAL && !mt.heads)
            return fail(h, GORDER_ERR_INVALID_ARGUMENT, "leaflets need heads[] per molecule type");
        if (lf.method == GORDER_LEAFLETS_INDIVIDUAL && (!mt.methyls || mt.n_methyls == 0))
            return fail(h, GORDER_ERR_INVALID_ARGUMENT, "individual leaflets need methyls[]");
        for (uint32_t k = 0; k < mt.n_molecules; k++) {
            const uint32_t hd = mt.heads ? mt.heads[k] : 0;
            if (hd >= t->n_atoms) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "head index out of range");
            heads.push_back(hd);
            if (lf.method == GORDER_LEAFLETS_INDIVIDUAL)
                for (uint32_t q = 0; q < mt.n_methyls; q++) {
                    const uint32_t a = mt.methyls[(size_t)k * mt.n_methyls + q];
                    if (a >= t->n_atoms) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "methyl index out of range");
                    ma.push_back(a);
                }
            mb.push_back((uint32_t)ma.size());
        }
    }
    ST_TRY(upload(h, h->d_heads, heads));
    h->host_heads = heads;
    if (lf.method == GORDER_LEAFLETS_LOCAL) {   // error key of a failed local centre: first slot of the molecule's type
        std::vector<uint32_t> ms;
        for (uint32_t m = 0; m < t->n_molecule_types; m++) ms.insert(ms.end(), t->molecule_types[m].n_molecules, p.slot0[m]);
        ST_TRY(upload(h, h->d_mol_slot0, ms));
    }
    ST_TRY(upload(h, h->d_methyl_begin, mb));
    ST_TRY(upload(h, h->d_methyl_atoms, ma));
    if (lf.method == GORDER_LEAFLETS_LOCAL && !(lf.radius > 0.0f))
        return fail(h, GORDER_ERR_INVALID_ARGUMENT, "local leaflets need a positive radius");
    if (lf.method == GORDER_LEAFLETS_GLOBAL || lf.method == GORDER_LEAFLETS_LOCAL) {
        if (!lf.membrane || lf.n_membrane == 0)
            return fail(h, GORDER_ERR_INVALID_ARGUMENT, "global/local leaflets need the membrane group");
        std::vector<uint32_t> mem(lf.membrane, lf.membrane + lf.n_membrane);
        for (uint32_t a : mem)
            if (a >= t->n_atoms) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "membrane index out of range");
        ST_TRY(upload(h, h->d_membrane, mem));
        h->membrane_is_frame = lf.n_membrane == t->n_atoms && !h->sw.leaflets_generic;       // (GORDER_HIP_LEAFLETS_GENERIC)
        for (uint32_t i = 0; i < lf.n_membrane && h->membrane_is_frame; i++) h->membrane_is_frame = mem[i] == i;
    }
    return GORDER_OK;
}

// the clustering methods' group "ClusterHeads" (leaflets.membrane) -> d_membrane, and every head's slot in it: each molecule's
// head is its own atom of the group (get_reference_head, leaflets.rs:1340-1345; an atom listed twice counts where it is first)
static int upload_cluster_group(gorder_hip_handle *h, const gorder_tables_t *t, const std::vector<uint32_t> &heads, bool ascending,
                                std::vector<uint32_t> &head_slot) {
    const gorder_leaflets_t &lf = t->leaflets;
    std::vector<uint32_t> grp(lf.membrane, lf.membrane + lf.n_membrane);
    std::vector<int32_t> slot_of(t->n_atoms, -1);       // atom -> slot in the group
    for (uint32_t i = 0; i < lf.n_membrane; i++) {
        if (grp[i] >= t->n_atoms) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "leaflets.membrane: index out of range");
        if (ascending && i && grp[i] <= grp[i - 1]) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "leaflets.membrane: clustering needs ascending, distinct atoms");
        if (slot_of[grp[i]] < 0) slot_of[grp[i]] = (int32_t)i;
    }
    for (uint32_t hd : heads) {
        if (slot_of[hd] < 0)
            return fail(h, GORDER_ERR_INVALID_ARGUMENT, "molecule_types[].heads: a head is not a member of leaflets.membrane");
        head_slot.push_back((uint32_t)slot_of[hd]);
    }
    return upload(h, h->d_membrane, grp);
}

static int create_spherical(gorder_hip_handle *h, const gorder_tables_t *t, const std::vector<uint32_t> &heads) {
    const gorder_leaflets_t &lf = t->leaflets;
    // leaflets.membrane is the group "ClusterHeads"; fewer than two atoms: NotEnoughAtomsToCluster (leaflets.rs:106-115)
    if (!lf.membrane || lf.n_membrane < 2)
        return fail(h, GORDER_ERR_INVALID_ARGUMENT, "leaflets.n_membrane: spherical clustering needs at least two group atoms");
    // (the kernel needs no molecule -> slot table on the device: it recomputes the head's distance and responsibility from the atom)
    std::vector<uint32_t> head_slot;
    ST_TRY(upload_cluster_group(h, t, heads, false, head_slot));
    // small groups: 256 threads a frame (16 atoms a thread, cheap barriers); larger ones 1024, and past
    // 16 x 1024 atoms a scratch row per frame of a launch — at most 64 MiB, whatever the batch
    h->sph_threads = lf.n_membrane <= 256u * (uint32_t)kSphKeep ? 256u : 1024u;
    const uint32_t resident = h->sph_threads * (uint32_t)kSphKeep;
    h->sph_spill = lf.n_membrane > resident ? lf.n_membrane - resident : 0u;
    if (h->sph_spill) {
        h->sph_slab = (uint32_t)std::min<size_t>(std::max<size_t>(((size_t)64 << 20) / (h->sph_spill * sizeof(float)), 1), 4096);
        if (h->sw.spherical_slab) h->sph_slab = std::min(h->sph_slab, h->sw.spherical_slab);      // (GORDER_HIP_SPHERICAL_SLAB, tests: only lowers the cap)
        ST_TRY(allocate(h, h->d_sph_spill, (size_t)h->sph_slab * h->sph_spill));
    }
    return allocate(h, h->d_sph_stats, 12, 0);
}

static int create_clustering(gorder_hip_handle *h, const gorder_tables_t *t, const std::vector<uint32_t> &heads) {
    const gorder_leaflets_t &lf = t->leaflets;
    // leaflets.membrane is the group "ClusterHeads" (leaflets.rs:96-105: at least two atoms); the dense route holds
    // n x (steps + 1) basis vectors a frame, hence the bound
    if (!lf.membrane || lf.n_membrane < kClMinGroup)
        return fail(h, GORDER_ERR_INVALID_ARGUMENT, "leaflets.n_membrane: clustering needs at least two group atoms");
    h->cl_cut = (t->flags & GORDER_FLAG_CLUSTER_CUTOFF) != 0;
    if (!h->cl_cut && lf.n_membrane > kClMaxGroup)
        return fail(h, GORDER_ERR_INVALID_ARGUMENT, "leaflets.n_membrane: clustering takes at most 8192 group atoms");
    if (h->cl_cut && lf.n_membrane > kClCutMaxGroup)
        return fail(h, GORDER_ERR_INVALID_ARGUMENT, "leaflets.n_membrane: clustering with GORDER_FLAG_CLUSTER_CUTOFF takes at most 131072 group atoms");
    std::vector<uint32_t> head_slot;
    ST_TRY(upload_cluster_group(h, t, heads, true, head_slot));
    ST_TRY(upload(h, h->d_cl_head_slot, head_slot));
    const uint32_t n = lf.n_membrane;
    h->cl_m_max = std::min<uint32_t>(n - 1u, (uint32_t)kClMaxSteps);
    // at most 512 MiB of scratch whatever the batch, at most 1024 frames a launch
    h->cl_tiles = (n + kClCutTile - 1u) / kClCutTile;
    h->cl_sort = (n + kClCutSort - 1u) / kClCutSort;
    const size_t per_frame = h->cl_cut ? clcut_frame_bytes(n, h->cl_m_max)
                                       : cl_frame_bytes(n, h->cl_m_max) + (h->sw.cluster_stored_w ? (size_t)n * n * 4 : 0);     // (GORDER_HIP_CLUSTER_STORED_W)
    h->cl_slab = (uint32_t)std::min<size_t>(std::max<size_t>(((size_t)512 << 20) / per_frame, 1), 1024);
    ST_TRY(allocate(h, h->d_cl_scratch, (size_t)h->cl_slab * per_frame));
    ST_TRY(allocate(h, h->d_cl_carry, n));
    ST_TRY(allocate(h, h->d_cl_is0, h->cl_slab));
    return allocate(h, h->d_cl_stats, 12, 0);
}

// one read for global leaflets + order parameters: the tables of k_bonds_tiled<..., MOM> and k_spec_fixup
static int create_speculation(gorder_hip_handle *h) {
    const Plan &p = h->plan;
    std::vector<uint2> own(p.tiles.size());
    for (size_t i = 0; i < own.size(); i++) own[i] = make_uint2(p.own[2 * i], p.own[2 * i + 1]);
    ST_TRY(upload(h, h->d_own, own));
    std::vector<std::vector<SpecSample>> per_mol(p.n_mol_total);
    for (const Tile &tile : p.tiles)
        for (uint32_t q = 0; q < tile.n_items; q++) {
            const Item &it = p.items[tile.item0 + q];
            per_mol[it.mol].push_back({tile.atom0 + it.li, tile.atom0 + it.lj, p.tile_slots[tile.slot0 + it.lslot]});
        }
    std::vector<uint32_t> mbeg(1, 0);
    std::vector<SpecSample> all;
    for (const auto &v : per_mol) { all.insert(all.end(), v.begin(), v.end()); mbeg.push_back((uint32_t)all.size()); }
    ST_TRY(upload(h, h->d_spec_mol_begin, mbeg));
    ST_TRY(upload(h, h->d_spec_samples, all));
    std::vector<uint2> oh(p.own_heads.size() / 2);
    for (size_t i = 0; i < oh.size(); i++) oh[i] = make_uint2(p.own_heads[2 * i], p.own_heads[2 * i + 1]);
    ST_TRY(upload(h, h->d_own_head_begin, p.own_head_begin));
    ST_TRY(upload(h, h->d_own_heads, oh));
    ST_TRY(allocate(h, h->d_spec_counters, 4, 0));
    ST_TRY(allocate(h, h->h_spec_counters, 2 * gorder_hip_handle::kSpecRing));
    for (Event &ev : h->spec_counters_copied) HIP_TRY(h, ev.create());
    h->spec_enabled = true;
    return GORDER_OK;
}

static int create_local_leaflets(gorder_hip_handle *h, const gorder_tables_t *t) {
    const Plan &p = h->plan;
    const size_t nm = t->leaflets.n_membrane, ncell = (size_t)kLocalMaxCells1D * kLocalMaxCells1D;
    const size_t sl = h->local_slab = local_slab_frames(nm, h->sw.local_slab);
    ST_TRY(local_build_attributes(h));
    // rows of cells with a halo (periodic boxes, k_local_flags_rows): the first cells of a row are there twice,
    // records included — room for twice the membrane
    h->local_halo = t->handle_pbc && !h->sw.local_atoms_only;
    h->local_rec_stride = (h->local_halo ? 2u : 1u) * nm;
    ST_TRY(allocate(h, h->d_lcell_of, sl * nm));
    ST_TRY(allocate(h, h->d_ltrig, sl * h->local_rec_stride * (sizeof(LocalRec) / sizeof(float))));
    ST_TRY(allocate(h, h->d_lcell_count, sl * (ncell + 1)));
    ST_TRY(allocate(h, h->d_lcell_fill, sl * ncell));
    ST_TRY(allocate(h, h->d_lgrid, sl));
    if (!h->local_halo) return GORDER_OK;   // (GORDER_HIP_LOCAL_ATOMS_ONLY, an A/B switch: every candidate atom by atom, the general passes)
    const size_t row_cells = sl * (size_t)kLocalMaxCells1D * (kLocalMaxCells1D + 1u);
    ST_TRY(allocate(h, h->d_lrowpre, row_cells));
    ST_TRY(allocate(h, h->d_ledge, row_cells));
    ST_TRY(allocate(h, h->d_lfinfo, sl));
    ST_TRY(allocate(h, h->d_lneed, sl + 1));
    ST_TRY(allocate(h, h->d_lsummary, 2, 0));
    ST_TRY(allocate(h, h->h_lsummary, 2));
    h->h_lsummary[0] = h->h_lsummary[1] = 0u;
    HIP_TRY(h, h->lsummary_written.create());
    HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void *>(k_local_decide), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kDecideLds));
    HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void *>(k_local_sums), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSumsLds));
    return allocate(h, h->d_ltodo, 1 + sl * (size_t)(p.n_mol_total ? p.n_mol_total : 1));
}

int gorder_hip_create(const gorder_tables_t *t, gorder_hip_handle **out) {
    if (!t || !out) return GORDER_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return GORDER_ERR_NO_DEVICE;
    if (t->device < 0 || t->device >= n_dev) return GORDER_ERR_INVALID_ARGUMENT;

    gorder_hip_handle *h = new (std::nothrow) gorder_hip_handle();
    if (!h) return GORDER_ERR_DEVICE;
    h->sw = gorder::read_switches(::getenv);      // the one look at the environment: whatever follows reads h->sw
    *out = h;   // returned even on failure so that the caller can read the message; destroy() is safe
    h->tables = *t;
    h->tables.molecule_types = nullptr;
    h->tables.leaflets.membrane = nullptr;
    h->device = t->device;
    HIP_TRY(h, hipSetDevice(h->device));
    if ((t->flags & GORDER_FLAG_UA_FAST_NORMALISE) && (t->flags & GORDER_FLAG_TRIG_ACOS_COS))
        return fail(h, GORDER_ERR_INVALID_ARGUMENT, "GORDER_FLAG_UA_FAST_NORMALISE (tolerance-bounded) and GORDER_FLAG_TRIG_ACOS_COS (literal) exclude each other");
    if ((t->flags & GORDER_FLAG_CLUSTER_CUTOFF) && t->leaflets.method != GORDER_LEAFLETS_CLUSTERING)
        return fail(h, GORDER_ERR_INVALID_ARGUMENT, "GORDER_FLAG_CLUSTER_CUTOFF needs leaflets.method == GORDER_LEAFLETS_CLUSTERING");
    // united atoms: a wave = 4 slots x 16 molecules (plan.h) — except for per-frame rows and nothing else, where a wave of
    // ONE slot sends a fourth of the atomics (0.433 against 0.449 ms per 3 000 frames of the 256-lipid membrane)
    const bool ua_rows_only = t->timewise && !t->ordermap.enabled && t->geometry.kind == GORDER_GEOM_NONE && !t->dynamic_normal.enabled;
    // (GORDER_HIP_FORCE_DIRECT, GORDER_HIP_UA_SLOT_WAVES)
    const int st = gorder::build_plan(*t, h->sw.force_direct, h->plan, !h->sw.ua_slot_waves && !ua_rows_only);
    if (st != GORDER_OK) return fail(h, st, "invalid bond tables");
    const Plan &p = h->plan;
    for (uint32_t m = 0; m < t->n_molecule_types; m++)
        h->map_max_mol = std::max(h->map_max_mol, t->molecule_types[m].n_molecules);
    HIP_TRY(h, h->own_stream.create());
    h->stream = h->own_stream;
    ST_TRY(upload(h, h->d_tiles, p.tiles));
    ST_TRY(upload(h, h->d_items, p.items));
    ST_TRY(upload(h, h->d_tile_slots, p.tile_slots));
    ST_TRY(upload(h, h->d_direct, p.direct));
    ST_TRY(upload(h, h->d_ua_tiles, p.ua_tiles));
    ST_TRY(upload(h, h->d_ua_items, p.ua_items));
    ST_TRY(upload(h, h->d_ua_tile_slots, p.ua_tile_slots));
    ExtraArgs &e = h->extra;
    // construction angles of the united-atom hydrogens (uaorder.rs:34-41); sin/cos with the host
    // libm, as the reference's nalgebra Rotation3::from_axis_angle does
    e.sin_tet = sinf(1.910633f); e.cos_tet = cosf(1.910633f);
    e.sin_ch3 = sinf(2.0943952f); e.cos_ch3 = cosf(2.0943952f);
    e.sin_half = sinf(0.9553165f); e.cos_half = cosf(0.9553165f);
    ST_TRY(create_ordermaps(h, t));
    e.tw = t->timewise ? 1 : 0;
    if (t->timewise && !p.tiles.empty()) {      // k_bonds_tiled_tw: the tile items in slot order and their runs
        if (!h->d_items_by_slot) ST_TRY(upload(h, h->d_items_by_slot, p.items_by_slot));
        ST_TRY(upload(h, h->d_item_run, p.item_run));
    }
    ST_TRY(create_geometry(h, t));
    if ((e.maps || e.tw || e.geom_kind) && !p.direct.empty())
        return fail(h, GORDER_ERR_INVALID_ARGUMENT, "ordermaps / timewise / geometry need every bond to fit an atom window");
    ST_TRY(create_accumulators(h));
    {   // |normal| with the f32 sequence of nalgebra's norm (oracle: norm3)
        const float *n = t->normal;
        h->n2sq = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
        h->n2 = sqrtf(h->n2sq);
        for (int d = 0; d < 3; d++)
            if (n[d] == 1.0f && n[(d + 1) % 3] == 0.0f && n[(d + 2) % 3] == 0.0f) h->axis = d;
        h->extra.axis = h->axis;
    }
    h->lw = ((3u * p.max_window + 3u + 3u) / 4u) * 4u;
    h->lds_bytes = (size_t)h->frames_per_stage * h->lw * sizeof(float);
    if (h->lds_bytes < (size_t)kBlock * 24) h->lds_bytes = (size_t)kBlock * 24;
    {   // how many workgroups of the tiled kernel are co-resident: the frame range of a batch is cut so
        // that the grid is a whole number of such rounds (no half-empty last round)
        int n_cu = 256, per_cu = 6;
        (void)hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, h->device);
        const bool ac = (t->flags & GORDER_FLAG_TRIG_ACOS_COS) != 0;
        const hipError_t e = ac ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_bonds_tiled<4, 5, true, true, false, -1>, kBlock, h->lds_bytes)
                                : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_bonds_tiled<4, 5, false, true, false, 2>, kBlock, h->lds_bytes);
        if (e != hipSuccess || per_cu < 1) per_cu = 4;
        h->wg_capacity = (uint32_t)n_cu * (uint32_t)per_cu;
    }
    ST_TRY(create_dynamic_normals(h, t));
    const gorder_leaflets_t &lf = t->leaflets;
    if (lf.method != GORDER_LEAFLETS_NONE) {
        std::vector<uint32_t> heads;
        ST_TRY(create_leaflet_tables(h, t, heads));
        if (lf.method == GORDER_LEAFLETS_SPHERICAL) ST_TRY(create_spherical(h, t, heads));
        if (lf.method == GORDER_LEAFLETS_CLUSTERING) ST_TRY(create_clustering(h, t, heads));
        if (lf.method == GORDER_LEAFLETS_GLOBAL && p.spec_ok && !h->sw.no_speculate) ST_TRY(create_speculation(h));
        if (lf.method == GORDER_LEAFLETS_LOCAL) ST_TRY(create_local_leaflets(h, t));
        ST_TRY(allocate(h, h->d_adist, p.n_mol_total ? p.n_mol_total : 1));
    }
    // the memsets above ran on the null stream, which the handle's non-blocking stream does not wait for
    HIP_TRY(h, hipDeviceSynchronize());
    return GORDER_OK;
}

void gorder_hip_destroy(gorder_hip_handle *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);      // (nothing is in flight when the buffers free themselves)
    if (h->traj_cache_free) h->traj_cache_free(h);
    delete h;      // every member frees what it owns (device_mem.h, Event, Stream, CollectStore)
}

uint32_t gorder_hip_n_accumulators(const gorder_hip_handle *h) { return h ? h->plan.n_acc : 0; }
uint32_t gorder_hip_ordermap_dims(const gorder_hip_handle *h, uint32_t *nx, uint32_t *ny) {
    if (nx) *nx = h ? h->map_nx : 0;
    if (ny) *ny = h ? h->map_ny : 0;
    return h ? h->map_nx * h->map_ny : 0;
}

int gorder_hip_set_stream(gorder_hip_handle *h, void *hip_stream) {
    if (!h) return GORDER_ERR_INVALID_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->stream = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
    return GORDER_OK;
}

static void spec_poll(gorder_hip_handle *h, bool wait);
int gorder_hip_speculation_stats(gorder_hip_handle *h, uint64_t out[4]) {
    if (!h || !out) return GORDER_ERR_INVALID_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    spec_poll(h, true);
    out[0] = h->spec_batches; out[1] = h->spec_fixed; out[2] = h->spec_exact_frames; out[3] = h->spec_enabled ? 1 : 0;
    return GORDER_OK;
}

int gorder_hip_local_decide_stats(gorder_hip_handle *h, uint64_t out[4]) {
    if (!h || !out) return GORDER_ERR_INVALID_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    out[0] = h->decide_submits; out[1] = h->decide_paused_submits;
    out[2] = h->h_lsummary ? h->h_lsummary[0] : 0; out[3] = h->h_lsummary ? h->h_lsummary[1] : 0;
    return GORDER_OK;
}

int gorder_hip_plan(const gorder_hip_handle *h, gorder_hip_plan_t *plan) {
    if (!h || !plan) return GORDER_ERR_INVALID_ARGUMENT;
    plan->n_tiles = (uint32_t)h->plan.tiles.size();
    plan->block_threads = kBlock;
    plan->max_window_atoms = h->plan.max_window;
    plan->n_direct_items = (uint32_t)h->plan.direct.size();
    plan->frames_per_stage = (uint32_t)h->frames_per_stage;
    plan->lds_bytes = (uint32_t)h->lds_bytes;
    plan->map_staged = h->map_staged ? 1u : 0u;
    plan->map_lds_bytes = (uint32_t)h->map_lds_bytes;
    plan->leaflets_one_read = h->plan.spec_ok ? 1u : 0u;
    return GORDER_OK;
}

// What the speculative batches that have finished cost (never waits unless `wait`): their counters are added to the
// handle's statistics, and a batch that left more than 1/8 of its frames to the exact kernel, or mispredicted more than
// 1/16 of its (frame, molecule) pairs, ends the speculation for this handle — a membrane across the periodic boundary,
// lipids that keep changing sides: the two-kernel path is the cheaper one for such a trajectory.
static void spec_poll(gorder_hip_handle *h, bool wait) {
    for (uint32_t i = 0; i < gorder_hip_handle::kSpecRing; i++) {
        if (!h->spec_ring_frames[i]) continue;
        if (wait) (void)hipEventSynchronize(h->spec_counters_copied[i]);
        else if (hipEventQuery(h->spec_counters_copied[i]) != hipSuccess) continue;
        const uint32_t moved = h->h_spec_counters[2 * i], exact = h->h_spec_counters[2 * i + 1];
        h->spec_fixed += moved;
        h->spec_exact_frames += exact;
        if ((uint64_t)exact * 8u > h->spec_ring_frames[i] ||
            (uint64_t)moved * 16u > h->spec_ring_frames[i] * h->plan.n_mol_total)
            h->spec_enabled = false;
        h->spec_ring_frames[i] = 0;
    }
}

// ---- leaflet assignment rows for a batch (host part of leaflets.rs:435-441, 1437-1472) --------
// spectral clustering: bytes of scratch one assignment frame takes (every array a multiple of 16 bytes), and the launch
static size_t cl_round(size_t b) { return (b + 15u) & ~(size_t)15u; }
static size_t cl_frame_bytes(uint32_t n, uint32_t m_max) {
    return cl_round(3 * (size_t)n * 4) + 3 * cl_round((size_t)n * 4) + cl_round((size_t)(m_max + 1u) * n * 4) +
           cl_round(kClSol * 8) + cl_round(n) + cl_round(kClMeta * 4) + 16;
}
// the cut-off route's arrays of one frame, in carving order: {bytes}
static void clcut_sizes(uint32_t n, uint32_t m_max, size_t (&b)[22]) {
    const size_t tiles = (n + kClCutTile - 1u) / kClCutTile, sort = (n + kClCutSort - 1u) / kClCutSort, nf = cl_round((size_t)n * 4);
    const size_t v[22] = {cl_round(kClSol * 8), cl_round((size_t)tiles * kClLd * 8), cl_round(kClLd * 8), cl_round(2 * kClLd * 8),
                          cl_round(kClCutScal * 8), cl_round(sizeof(ClCutGrid)), cl_round(sort * kClCutMaxCells * 4),
                          cl_round((kClCutMaxCells + 1u) * 4), nf /* cell_of */, nf /* perm */, cl_round(3 * (size_t)n * 4), nf /* s */,
                          nf /* q */, nf /* emb */, nf /* e0 */, nf /* e1 */, cl_round((size_t)(m_max + 1u) * n * 4),
                          cl_round(kClMeta * 4), 16 /* fail */, 16 /* done */, cl_round(n) /* lab */, 0};
    for (int k = 0; k < 22; k++) b[k] = v[k];
}
static size_t clcut_frame_bytes(uint32_t n, uint32_t m_max) {
    size_t b[22], sum = 0;
    clcut_sizes(n, m_max, b);
    for (size_t v : b) sum += v;
    return sum;
}
// GORDER_FLAG_CLUSTER_CUTOFF: the launches of kernels_cluster_cutoff.h.  The whole step budget is queued; a frame that has
// converged sets its `done` word on the device and its workgroups leave at once — nothing is read back here.
static int run_clustering_cutoff(gorder_hip_handle *h, const float *d_xyz, const float *d_box, size_t n_assign, uint32_t row0) {
    const gorder_leaflets_t &lf = h->tables.leaflets;
    const uint32_t n = lf.n_membrane, slab = h->cl_slab, tiles = h->cl_tiles, sort = h->cl_sort;
    size_t bytes[22];
    clcut_sizes(n, h->cl_m_max, bytes);
    ClCutArgs ca{};
    ca.c.xyz = d_xyz; ca.c.box9 = d_box; ca.c.n_atoms = h->plan.n_atoms; ca.c.group = h->d_membrane; ca.c.n = n;
    ca.c.pbc = h->tables.handle_pbc ? 1 : 0; ca.c.m_max = h->cl_m_max; ca.c.err = h->d_err; ca.c.W = nullptr;
    ca.n_tiles = tiles; ca.n_sort = sort;
    char *base = (char *)h->d_cl_scratch;
    int at = 0;
    auto carve = [&]() { char *p = base; base += bytes[at++] * slab; return p; };
    ca.c.sol = (double *)carve(); ca.part = (double *)carve(); ca.coef = (double *)carve(); ca.albe = (double *)carve();
    ca.scal = (double *)carve(); ca.grid = (ClCutGrid *)carve(); ca.cnt = (uint32_t *)carve(); ca.cell_start = (uint32_t *)carve();
    ca.cell_of = (uint32_t *)carve(); ca.perm = (uint32_t *)carve(); ca.c.pos = (float *)carve(); ca.c.s = (float *)carve();
    ca.c.q = (float *)carve(); ca.c.emb = (float *)carve(); ca.e0 = (float *)carve(); ca.e1 = (float *)carve();
    ca.c.V = (float *)carve(); ca.c.meta = (float *)carve(); ca.c.fail = (uint32_t *)carve(); ca.done = (uint32_t *)carve();
    ca.c.lab = (uint8_t *)carve();
    ClOrientArgs oa{};
    oa.n = n; oa.lab = ca.c.lab; oa.emb = ca.c.emb; oa.meta = ca.c.meta; oa.fail = ca.c.fail; oa.carry = h->d_cl_carry;
    oa.aflags = h->d_aflags; oa.n_mol_total = h->plan.n_mol_total; oa.head_slot = h->d_cl_head_slot;
    oa.flip = lf.flip ? 1 : 0; oa.err = h->d_err; oa.is_frame0 = h->d_cl_is0;
    for (size_t done = 0; done < n_assign; done += slab) {
        const uint32_t ns = (uint32_t)std::min<size_t>(n_assign - done, slab);
        const bool last = done + ns == n_assign;
        ca.c.aframes = h->d_aframes + done; ca.c.n_assign = ns;
        oa.aframes = ca.c.aframes; oa.n_assign = ns; oa.row0 = row0 + (uint32_t)done;
        oa.adist = last ? h->d_adist : nullptr;
        oa.stats = last ? h->d_cl_stats : nullptr;
        const dim3 rows(tiles, ns), blocks(sort, ns);
        HIP_TRY(h, hipMemsetAsync(ca.c.fail, 0, (size_t)ns * sizeof(uint32_t), h->stream));
        HIP_TRY(h, hipMemsetAsync(ca.done, 0, (size_t)ns * sizeof(uint32_t), h->stream));
        HIP_TRY(h, hipMemcpyAsync(h->d_cl_is0, h->cl_is0.data() + done, ns, hipMemcpyHostToDevice, h->stream));
        TIMING_MARK(h, "k_clcut_cells");
        hipLaunchKernelGGL(k_clcut_grid, dim3(ns), dim3(256), 0, h->stream, ca);
        hipLaunchKernelGGL(k_clcut_count, blocks, dim3(1024), 0, h->stream, ca);
        hipLaunchKernelGGL(k_clcut_scan, dim3(ns), dim3(1024), 0, h->stream, ca);
        hipLaunchKernelGGL(k_clcut_scatter, blocks, dim3(1024), 0, h->stream, ca);
        TIMING_MARK(h, "k_clcut_lanczos");
        hipLaunchKernelGGL(k_clcut_degrees, rows, dim3(kClCutTile), 0, h->stream, ca);
        hipLaunchKernelGGL(k_clcut_start, dim3(ns), dim3(1024), 0, h->stream, ca);
        for (int j = 0; j < (int)h->cl_m_max; j++) {
            hipLaunchKernelGGL(k_clcut_spmv, rows, dim3(kClCutTile), 0, h->stream, ca, j);
            hipLaunchKernelGGL(k_clcut_coef, dim3(ns), dim3(512), 0, h->stream, ca, j, 0);
            hipLaunchKernelGGL(k_clcut_update, rows, dim3(kClCutTile), 0, h->stream, ca, j, 0);
            hipLaunchKernelGGL(k_clcut_dots, rows, dim3(kClCutTile), 0, h->stream, ca, j);
            hipLaunchKernelGGL(k_clcut_coef, dim3(ns), dim3(512), 0, h->stream, ca, j, 1);
            hipLaunchKernelGGL(k_clcut_update, rows, dim3(kClCutTile), 0, h->stream, ca, j, 1);
            hipLaunchKernelGGL(k_clcut_small, dim3(ns), dim3(1024), 0, h->stream, ca, j);
            hipLaunchKernelGGL(k_clcut_scale, rows, dim3(kClCutTile), 0, h->stream, ca, j);
        }
        TIMING_MARK(h, "k_clcut_embed");
        hipLaunchKernelGGL(k_clcut_ritz, rows, dim3(kClCutTile), 0, h->stream, ca);
        hipLaunchKernelGGL(k_clcut_embed, dim3(ns), dim3(1024), 0, h->stream, ca);
        TIMING_MARK(h, "k_cluster_orient");
        hipLaunchKernelGGL(k_cluster_orient, dim3(1), dim3(1024), 0, h->stream, oa);
        HIP_TRY(h, hipGetLastError());
    }
    h->cl_have_carry = true;
    return GORDER_OK;
}

static int run_clustering(gorder_hip_handle *h, const float *d_xyz, const float *d_box, size_t n_assign, uint32_t row0) {
    if (h->cl_cut) return run_clustering_cutoff(h, d_xyz, d_box, n_assign, row0);
    const gorder_leaflets_t &lf = h->tables.leaflets;
    const uint32_t n = lf.n_membrane, slab = h->cl_slab;
    ClArgs ca{};
    ca.xyz = d_xyz; ca.box9 = d_box; ca.n_atoms = h->plan.n_atoms; ca.group = h->d_membrane; ca.n = n;
    ca.pbc = h->tables.handle_pbc ? 1 : 0; ca.m_max = h->cl_m_max; ca.err = h->d_err;
    char *base = (char *)h->d_cl_scratch;
    auto carve = [&](size_t per_frame) { char *at = base; base += per_frame * slab; return at; };
    ca.sol = (double *)carve(cl_round(kClSol * 8));
    ca.pos = (float *)carve(cl_round(3 * (size_t)n * 4));
    ca.s = (float *)carve(cl_round((size_t)n * 4));
    ca.q = (float *)carve(cl_round((size_t)n * 4));
    ca.emb = (float *)carve(cl_round((size_t)n * 4));
    ca.V = (float *)carve(cl_round((size_t)(h->cl_m_max + 1u) * n * 4));
    ca.meta = (float *)carve(cl_round(kClMeta * 4));
    ca.fail = (uint32_t *)carve(16);
    ca.lab = (uint8_t *)carve(cl_round(n));
    ca.W = h->sw.cluster_stored_w ? (float *)carve((size_t)n * n * 4) : nullptr;
    // (the arrays are indexed [slot][..] with their exact sizes: the rounding only pads the ends)
    ClOrientArgs oa{};
    oa.n = n; oa.lab = ca.lab; oa.emb = ca.emb; oa.meta = ca.meta; oa.fail = ca.fail; oa.carry = h->d_cl_carry;
    oa.aflags = h->d_aflags; oa.n_mol_total = h->plan.n_mol_total; oa.head_slot = h->d_cl_head_slot;
    oa.flip = lf.flip ? 1 : 0; oa.err = h->d_err; oa.is_frame0 = h->d_cl_is0;
    for (size_t done = 0; done < n_assign; done += slab) {
        const uint32_t ns = (uint32_t)std::min<size_t>(n_assign - done, slab);
        const bool last = done + ns == n_assign;
        ca.aframes = h->d_aframes + done; ca.n_assign = ns;
        oa.aframes = ca.aframes; oa.n_assign = ns; oa.row0 = row0 + (uint32_t)done;
        oa.adist = last ? h->d_adist : nullptr;
        oa.stats = last ? h->d_cl_stats : nullptr;
        HIP_TRY(h, hipMemsetAsync(ca.fail, 0, (size_t)ns * sizeof(uint32_t), h->stream));
        HIP_TRY(h, hipMemcpyAsync(h->d_cl_is0, h->cl_is0.data() + done, ns, hipMemcpyHostToDevice, h->stream));
        TIMING_MARK(h, "k_cluster_degrees");
        hipLaunchKernelGGL(k_cluster_degrees, dim3((n + 255u) / 256u, ns), dim3(256), 0, h->stream, ca);
        TIMING_MARK(h, "k_cluster_lanczos");
        hipLaunchKernelGGL(k_cluster_lanczos, dim3(ns), dim3(1024), 0, h->stream, ca);
        TIMING_MARK(h, "k_cluster_embed");
        hipLaunchKernelGGL(k_cluster_embed, dim3(ns), dim3(1024), 0, h->stream, ca);
        TIMING_MARK(h, "k_cluster_orient");
        hipLaunchKernelGGL(k_cluster_orient, dim3(1), dim3(1024), 0, h->stream, oa);
    }
    h->cl_have_carry = true;
    return GORDER_OK;
}

// ---- the kernels of la.n_assign assignment frames, a function per method; `la` is what run_leaflets (below) filled in
static int launch_global_leaflets(gorder_hip_handle *h, const LeafletArgs &la) {
    // (behind a speculative batch nearly every frame is skipped: a few hundred workgroups take the frames in turn)
    const dim3 g(la.skip ? std::min<uint32_t>(la.n_assign, 512u) : la.n_assign), b(1024);
    TIMING_MARK(h, h->membrane_is_frame ? "k_leaflets_global_contig" : "k_leaflets_global");
    if (h->membrane_is_frame) {
        if (la.skip) hipLaunchKernelGGL(k_leaflets_global_contig<true>, g, dim3(256), 0, h->stream, la);
        else hipLaunchKernelGGL(k_leaflets_global_contig<false>, g, dim3(256), 0, h->stream, la);
    } else {
        if (la.skip) hipLaunchKernelGGL(k_leaflets_global<true>, g, b, 0, h->stream, la);
        else hipLaunchKernelGGL(k_leaflets_global<false>, g, b, 0, h->stream, la);
    }
    return GORDER_OK;
}

static int launch_individual_leaflets(gorder_hip_handle *h, const LeafletArgs &la) {
    // gridDim.y <= 65535: launch in slabs
    TIMING_MARK(h, "k_leaflets_individual");
    for (uint32_t done = 0; done < la.n_assign;) {
        const uint32_t ny = std::min<uint32_t>(la.n_assign - done, 65535u);
        LeafletArgs lb = la;
        lb.aframes = la.aframes + done;
        lb.row0 = la.row0 + done;
        // adist is only written by the last slab's last row
        if (done + ny < la.n_assign) lb.adist = nullptr;
        hipLaunchKernelGGL(k_leaflets_individual, dim3((la.n_mol_total + 255) / 256, ny), dim3(256), 0,
                           h->stream, lb);
        done += ny;
    }
    return GORDER_OK;
}

static int launch_spherical_leaflets(gorder_hip_handle *h, const LeafletArgs &la) {
    // a workgroup per assignment frame; a group too large for the registers goes in slabs of frames (scratch rows)
    TIMING_MARK(h, "k_leaflets_spherical");
    SphArgs sa{};
    sa.xyz = la.xyz; sa.box9 = la.box9; sa.n_atoms = la.n_atoms;
    sa.aflags = la.aflags; sa.n_mol_total = la.n_mol_total; sa.heads = la.heads;
    sa.group = la.membrane; sa.n_group = la.n_membrane;
    sa.flip = la.flip; sa.pbc = la.pbc;
    sa.spill = h->d_sph_spill; sa.n_spill = h->sph_spill; sa.err = la.err;
    for (size_t done = 0; done < la.n_assign; done += h->sph_slab) {
        const uint32_t ns = (uint32_t)std::min<size_t>(la.n_assign - done, h->sph_slab);
        const bool last = done + ns == la.n_assign;
        sa.aframes = la.aframes + done;
        sa.row0 = la.row0 + (uint32_t)done;
        sa.n_assign = ns;
        sa.adist = last ? h->d_adist : nullptr;
        sa.stats = last ? h->d_sph_stats : nullptr;
        if (h->sph_threads == 256u) hipLaunchKernelGGL(k_leaflets_spherical<256>, dim3(ns), dim3(256), 0, h->stream, sa);
        else hipLaunchKernelGGL(k_leaflets_spherical<1024>, dim3(ns), dim3(1024), 0, h->stream, sa);
    }
    return GORDER_OK;
}

// Local leaflets, what this submit runs.  decide: the bound first, a lane per head (k_local_decide), the rows kernel then only
// for the frames with a head left open; sums: the table that kernel reads made from per-cell sums first (k_local_sums), the cell
// list only for the frames left open; report: this submit writes {frames left open, frames} for a later one to read.
struct LocalDecisions { bool decide, sums, report; };
static LocalDecisions local_decisions(gorder_hip_handle *h, const LocalArgs &lo) {
    LocalDecisions d{};
    d.decide = lo.halo && lo.prune && lo.n_mol_total && !h->sw.local_no_decide;      // (GORDER_HIP_LOCAL_NO_DECIDE)
    if (d.decide) {
        if (h->lsummary_pending) {
            if (hipEventQuery(h->lsummary_written) == hipSuccess) {
                h->lsummary_pending = false;
                if (2u * h->h_lsummary[0] > h->h_lsummary[1]) h->decide_pause = gorder_hip_handle::kDecidePause;
            } else {
                (void)hipGetLastError();        // (hipErrorNotReady is an answer, not a failure of this submit)
            }
        }
        if (h->decide_pause) { h->decide_pause--; h->decide_paused_submits++; d.decide = false; }
        else h->decide_submits++;
    }
    d.sums = d.decide && lo.n_membrane <= kLocalBuildMax && !h->sw.local_three_kernels && !h->sw.local_no_sums;      // (GORDER_HIP_LOCAL_NO_SUMS)
    d.report = d.decide && !h->lsummary_pending;      // (one report in flight)
    return d;
}

// ... and its kernels, local_slab assignment frames at a time
static int launch_local_slabs(gorder_hip_handle *h, LocalArgs lo, uint32_t n_assign, uint32_t row0, bool report) {
    const size_t ncell = (size_t)kLocalMaxCells1D * kLocalMaxCells1D;
    for (size_t done = 0; done < n_assign; done += h->local_slab) {
        const uint32_t ns = (uint32_t)std::min<size_t>(n_assign - done, h->local_slab);
        lo.aframes = h->d_aframes + done;
        lo.n_slab = ns;
        lo.row0 = row0 + (uint32_t)done;
        lo.write_dist_frame = (done + ns == n_assign) ? (int)ns - 1 : -1;
        lo.summary_host = report && done + ns == n_assign ? h->h_lsummary : nullptr;
        if (lo.n_membrane > kLocalBuildMax || h->sw.local_three_kernels)
            HIP_TRY(h, hipMemsetAsync(h->d_lcell_fill, 0, ns * ncell * sizeof(uint32_t), h->stream));
        if (lo.sums) {
            HIP_TRY(h, hipMemsetAsync(h->d_lneed, 0, (ns + 1) * sizeof(uint32_t), h->stream));
            TIMING_MARK(h, "k_local_sums");
            hipLaunchKernelGGL(k_local_sums, dim3(ns), dim3(1024), kSumsLds, h->stream, lo);
            TIMING_MARK(h, "k_local_decide");
            hipLaunchKernelGGL(k_local_decide, dim3(ns), dim3(1024), kDecideLds, h->stream, lo);
        }
        ST_TRY(launch_cell_list(h, lo, ns, lo.n_membrane, h->d_lcell_count, ns * (ncell + 1) * sizeof(uint32_t)));
        if (lo.halo) {
            TIMING_MARK(h, "k_local_rowprefix");
            hipLaunchKernelGGL(k_local_rowprefix, dim3(kLocalMaxCells1D / 4u, ns), dim3(256), 0, h->stream, lo);
            lo.rows_groups = (lo.n_mol_total + 15u) / 16u;
            if (lo.need && !lo.sums) {
                TIMING_MARK(h, "k_local_decide");
                hipLaunchKernelGGL(k_local_decide, dim3(ns), dim3(1024), kDecideLds, h->stream, lo);
            }
            TIMING_MARK(h, "k_local_flags_rows");
            if (lo.need) hipLaunchKernelGGL(k_local_flags_rows_open, dim3(lo.rows_groups * 8u * kRowsSlots), dim3(256), 0, h->stream, lo);
            else hipLaunchKernelGGL(k_local_flags_rows, dim3(lo.rows_groups * ((ns + 7u) / 8u * 8u)), dim3(256), 0, h->stream, lo);
            // the heads the rows left over (normally none: the grid finds an empty list and leaves)
            TIMING_MARK(h, "k_local_flags_todo");
            hipLaunchKernelGGL(k_local_flags_todo, dim3(512), dim3(256), 0, h->stream, lo);
        } else {
            TIMING_MARK(h, "k_local_flags");
            hipLaunchKernelGGL(k_local_flags, dim3((lo.n_mol_total + 3) / 4, ns), dim3(256), 0, h->stream, lo);
        }
    }
    return GORDER_OK;
}

static int launch_local_leaflets(gorder_hip_handle *h, const LeafletArgs &la) {
    const gorder_leaflets_t &lf = h->tables.leaflets;
    LocalArgs lo{};
    lo.xyz = la.xyz; lo.box9 = la.box9; lo.n_atoms = la.n_atoms;
    lo.aflags = la.aflags; lo.adist = la.adist; lo.n_mol_total = la.n_mol_total;
    lo.heads = la.heads; lo.mol_slot0 = h->d_mol_slot0; lo.n_membrane = la.n_membrane;
    lo.membrane = h->membrane_is_frame ? nullptr : h->d_membrane;      // (the whole frame in order: no index list)
    lo.dim = la.dim; lo.flip = la.flip; lo.pbc = la.pbc;
    lo.radius = lf.radius;
    lo.radius_thr = local_radius_threshold(lf.radius);
    lo.cell_of = h->d_lcell_of; lo.trig = h->d_ltrig; lo.cell_count = h->d_lcell_count;
    lo.cell_fill = h->d_lcell_fill; lo.err = la.err;
    lo.grid = h->d_lgrid;
    lo.halo = h->local_halo ? 1 : 0;
    lo.prune = h->sw.local_no_prune ? 0 : (h->sw.local_decide_nothing ? 2 : 1);
    lo.rec_stride = (uint32_t)h->local_rec_stride;
    lo.rowpre = h->d_lrowpre;
    lo.edge = h->d_ledge;
    lo.finfo = h->d_lfinfo;
    lo.todo = h->d_ltodo;
    const LocalDecisions d = local_decisions(h, lo);
    lo.need = d.decide ? h->d_lneed : nullptr;
    lo.sums = d.sums ? 1 : 0;
    lo.summary = d.report ? h->d_lsummary : nullptr;
    ST_TRY(launch_local_slabs(h, lo, la.n_assign, la.row0, d.report));
    if (d.report) {
        HIP_TRY(h, hipEventRecord(h->lsummary_written, h->stream));
        h->lsummary_pending = true;
    }
    return GORDER_OK;
}

// The sides of the assignment frames `aframes` (positions in the batch) -> rows row0.. of d_aflags; `skip`: per frame, nothing to do
static int run_leaflets(gorder_hip_handle *h, const float *d_xyz, const float *d_box,
                        const std::vector<uint32_t> &aframes, uint32_t row0, const uint8_t *skip = nullptr) {
    if (aframes.empty()) return GORDER_OK;
    ST_TRY(upload_if_changed(h, h->d_aframes, h->up_aframes, h->up_aframes_valid, aframes));
    const gorder_leaflets_t &lf = h->tables.leaflets;
    LeafletArgs la{};
    la.xyz = d_xyz; la.box9 = d_box; la.n_atoms = h->plan.n_atoms;
    la.aframes = h->d_aframes; la.row0 = row0; la.aflags = h->d_aflags; la.adist = h->d_adist;
    la.n_mol_total = h->plan.n_mol_total; la.heads = h->d_heads;
    la.membrane = h->d_membrane; la.n_membrane = lf.n_membrane;
    la.methyl_begin = h->d_methyl_begin; la.methyl_atoms = h->d_methyl_atoms;
    la.dim = lf.normal_dim; la.flip = lf.flip ? 1 : 0; la.pbc = h->tables.handle_pbc ? 1 : 0;
    la.err = h->d_err;
    la.skip = skip;
    la.n_assign = (uint32_t)aframes.size();
    switch (lf.method) {
    case GORDER_LEAFLETS_GLOBAL: ST_TRY(launch_global_leaflets(h, la)); break;
    case GORDER_LEAFLETS_INDIVIDUAL: ST_TRY(launch_individual_leaflets(h, la)); break;
    case GORDER_LEAFLETS_SPHERICAL: ST_TRY(launch_spherical_leaflets(h, la)); break;
    case GORDER_LEAFLETS_CLUSTERING: ST_TRY(run_clustering(h, d_xyz, d_box, aframes.size(), row0)); break;
    case GORDER_LEAFLETS_LOCAL: ST_TRY(launch_local_leaflets(h, la)); break;
    default: break;
    }
    HIP_TRY(h, hipGetLastError());
    return GORDER_OK;
}

// ---- bond reorientation: the batch's bond vectors into the ring, then every pair (frame, frame - lag), a sub-range at a time
static int launch_bond_corr(gorder_hip_handle *h, const FrameArgs &a) {
    BondCorr &bc = h->corr;
    const Plan &p = h->plan;
    const uint32_t n_tiles = (uint32_t)p.tiles.size(), n_lags = (uint32_t)bc.lags.size(), max_lag = bc.lags.back();
    if (!bc.ring) {      // the first batch: the sub-range is fixed here (the setter has checked that one frame fits)
        const uint64_t fit = gorder::corr_subrange_fit(gorder::corr_plane_bytes(n_tiles, kBlock), max_lag, gorder::kCorrRingBudget);
        bc.subrange = gorder::corr_subrange(fit, a.n_frames, h->sw.corr_subrange);      // (GORDER_HIP_CORR_SUBRANGE)
        bc.ring_planes = gorder::corr_ring_planes(max_lag, bc.subrange);
        bc.plane_items = n_tiles * kBlock;
        ST_TRY(allocate(h, bc.ring, (size_t)bc.ring_planes * bc.plane_items));
    }
    CorrArgs c{};
    c.ring = bc.ring; c.ring_planes = bc.ring_planes; c.plane_items = bc.plane_items;
    c.base = gorder::corr_plane_of(bc.seen, bc.ring_planes);
    c.history = (uint32_t)std::min<uint64_t>(bc.seen, GORDER_CORR_MAX_LAG);
    c.n_lags = n_lags; c.lags = bc.d_lags; c.rep = bc.acc.rep; c.n_rep = bc.acc.n_rep; c.n_acc = p.n_acc;
    c.leaflets = a.leaflets; c.aflags = a.aflags; c.arow = a.arow; c.n_mol_total = a.n_mol_total;
    c.xyz = a.xyz; c.box9 = a.box9; c.n_atoms = a.n_atoms; c.pbc = a.pbc;
    for (uint32_t lo = 0; lo < a.n_frames; lo += bc.subrange) {
        const uint32_t hi = (uint32_t)std::min<uint64_t>(a.n_frames, (uint64_t)lo + bc.subrange), nf = hi - lo;
        const gorder::CorrChunks ch = gorder::corr_chunks(nf, n_tiles, h->sw.wg_target, h->wg_capacity);
        const uint32_t n_groups = (n_lags + gorder::kCorrLagBlock - 1u) / gorder::kCorrLagBlock;
        const uint64_t grid = (uint64_t)n_tiles * ch.n_chunks * (h->sw.corr_grid_chunks ? 1u : n_groups);
        if ((uint64_t)n_tiles * nf > 0x7fffffffull || grid > 0x7fffffffull) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "batch too large");
        c.frame0 = lo; c.n_frames = hi; c.frames_per_chunk = ch.frames_per_chunk; c.n_chunks = h->sw.corr_grid_chunks ? 0u : ch.n_chunks;
        TIMING_MARK(h, "k_bond_units");
        hipLaunchKernelGGL(k_bond_units, dim3(n_tiles * nf), dim3(kBlock), 0, h->stream, c, h->d_tiles, h->d_items, n_tiles);
        TIMING_MARK(h, "k_bond_corr");
        hipLaunchKernelGGL((k_bond_corr<gorder::kCorrLagBlock>), dim3((uint32_t)grid), dim3(kBlock), 0, h->stream, c, h->d_tiles,
                           h->d_items, h->d_tile_slots, n_tiles);
        HIP_TRY(h, hipGetLastError());
    }
    return GORDER_OK;
}

// Room for `need` rows of n_mol_total flags in d_aflags.  A block that holds them stays; otherwise a block of `alloc_rows`
// rows takes its place, with keep_row0 behind a stream-ordered copy of row 0 (the assignment earlier batches left).
static int ensure_flag_rows(gorder_hip_handle *h, size_t need, size_t alloc_rows, bool keep_row0) {
    if (need <= h->aflags_rows) return GORDER_OK;
    const size_t n_mol = h->plan.n_mol_total;
    DBuf<uint8_t> nb;      // (adopted once the copy is through)
    ST_TRY(allocate(h, nb, alloc_rows * n_mol));
    if (keep_row0 && h->d_aflags) {
        // stream-ordered: the handle's stream is non-blocking, a null-stream copy would not be
        HIP_TRY(h, hipMemcpyAsync(nb, h->d_aflags, n_mol, hipMemcpyDeviceToDevice, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    h->d_aflags.swap(nb);
    h->aflags_rows = alloc_rows;
    return GORDER_OK;
}

// ---- one batch: what the stages of gorder_hip_submit_device hand to one another.  It lives on that function's stack and
// holds what used to be its locals; nothing in here outlives the call.
namespace {
struct Batch {
    const float *d_xyz, *d_box;
    const uint64_t *frame_index;
    uint32_t n_frames;
    bool pbc = false, leaflets = false;
    bool ltable = false;                        // the flag rows come from the whole-trajectory manual table
    gorder::ReplayLeafletBatch replay;          // ... as this plan has them
    std::vector<uint32_t> normal_rows;          // manual normal table: the row of every frame
    std::vector<uint32_t> arow, aframes;        // leaflet_rows.h
    std::vector<uint32_t> spec_aframes;         // a speculative batch: the frames whose exact sides follow the order kernel
    std::vector<uint64_t> collect_frames;       // collected leaflets: the assignment frames of this batch = rows 1.. of d_aflags
    uint64_t last_assign_frame = 0;
    size_t n_new_rows = 0;                      // flag rows this batch wrote behind row 0; the last becomes the carry
    uint64_t mol_rows_before = 0;
    gorder::OrderRouteIn ri;
    gorder::OrderRoute route;                   // what the order pass runs (order_route.h), decided before the first kernel is queued
    FrameArgs a{};

    // The exit for a failure after the first kernel of the batch is queued: a key its kernels raised is not committed under
    // the next batch's ordinal, and the batch appends no per-molecule rows.
    int abort_batch(gorder_hip_handle *h, int status) const {
        h->mol_store.truncate(mol_rows_before);
        hipLaunchKernelGGL(k_batch_abort, dim3(1), dim3(1), 0, h->stream, h->d_err);
        (void)hipGetLastError();
        (void)timing_mark(h, nullptr);
        return status;
    }
};
// a stage's step behind the first kernel of the batch: a failure leaves through abort_batch (ST_TRY and HIP_TRY: it simply returns)
#define BATCH_TRY(expr)                                                 \
    do {                                                                \
        const int bst_ = (expr);                                        \
        if (bst_ != GORDER_OK) return b.abort_batch(h, bst_);           \
    } while (0)
}  // namespace

// 1. what can refuse the batch before anything is queued: the overflow bound, the normals handed over for it, the tables' rows
static int check_batch(gorder_hip_handle *h, Batch &b) {
    const gorder_leaflets_t &lf = h->tables.leaflets;
    // OrderValue is a checked i64 (order.rs:44-60 panics on overflow).  |tick| <= 1e6 and a slot receives at most one
    // sample per molecule of its type and frame, so no sum can overflow while frames * molecules stays below 2^63 / 1e6:
    // refuse the batch that would cross that bound instead of wrapping silently.
    if ((h->n_frames + b.n_frames) > (uint64_t)(9223372036854775807ll / 1000000ll) / h->map_max_mol)
        return fail(h, GORDER_ERR_OVERFLOW, "order accumulators could overflow i64 (frames x molecules >= 2^63 / 1e6)");
    if (h->manual_frames) {
        if (h->manual_frames != b.n_frames) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_set_normals: frame count differs from the batch");
        if (!h->plan.direct.empty()) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "manual normals: a bond spans more than the LDS window");
    }
    // whole-trajectory manual tables: every frame of the batch must have its row, or the batch is refused whole
    b.ltable = lf.method == GORDER_LEAFLETS_MANUAL && h->d_ltable;
    uint64_t bad = 0;
    if (b.ltable && gorder::replay_plan_leaflets(lf.frequency, h->ltable_win, h->replay_have_carry, h->replay_carry_index, b.frame_index,
                                                 b.n_frames, b.replay, &bad) != gorder::kReplayOk) {
        h->err_frame = bad;
        return fail(h, GORDER_ERR_MANUAL_LEAFLET_FRAME, "manual leaflet table: no row for frame " + std::to_string(bad));
    }
    if (h->d_ntable) {
        const gorder::ReplayStatus rs = gorder::replay_plan_normals(h->ntable_step, h->ntable_win, b.frame_index, b.n_frames, b.normal_rows, &bad);
        if (rs != gorder::kReplayOk) {
            h->err_frame = bad;
            if (rs == gorder::kReplayBadStep)
                return fail(h, GORDER_ERR_INVALID_ARGUMENT, "manual normal table: frame " + std::to_string(bad) + " is no multiple of the step");
            return fail(h, GORDER_ERR_MANUAL_NORMAL_FRAME, "manual normal table: no row for frame " + std::to_string(bad));
        }
    }
    return GORDER_OK;
}

// 2. the row of the flag block every frame is routed by (leaflet_rows.h; a table: replay_rows.h has planned them in 1.)
static int plan_batch_rows(gorder_hip_handle *h, Batch &b) {
    const gorder_leaflets_t &lf = h->tables.leaflets;
    b.last_assign_frame = h->assignment_frame;
    if (!b.leaflets) return GORDER_OK;
    if (b.ltable) {
        b.arow = b.replay.arow;
        b.last_assign_frame = b.replay.carry_index * lf.frequency;       // the assignment frame of the newest row
        return GORDER_OK;
    }
    switch (gorder::plan_assignment_rows(lf.method, lf.frequency, h->have_assignment, h->cl_have_carry, b.frame_index, b.n_frames,
                                         b.arow, b.aframes, h->cl_is0, b.last_assign_frame)) {
    case gorder::kLeafletRowsNoClusters:
        return fail(h, GORDER_ERR_LEAFLETS_NOT_PRIMED, "clustering: no clusters of an earlier assignment frame to match against");
    case gorder::kLeafletRowsNotPrimed:
        return fail(h, GORDER_ERR_LEAFLETS_NOT_PRIMED, "no leaflet assignment for the first frame");
    default: return GORDER_OK;
    }
}

// 3. what the order pass will run.  One read for global leaflets + order parameters (route.speculative): the order kernel
// then routes by row 0; the counters of earlier speculative batches are looked at first, and may turn it off.
static void choose_batch_route(gorder_hip_handle *h, Batch &b) {
    const Plan &p = h->plan;
    gorder::OrderRouteIn &ri = b.ri;
    ri.acos = (h->tables.flags & GORDER_FLAG_TRIG_ACOS_COS) != 0; ri.pbc = b.pbc; ri.leaflets = b.leaflets; ri.axis = h->axis;
    ri.maps = h->extra.maps != 0; ri.map_staged = h->map_staged; ri.tw = h->extra.tw != 0; ri.geom = h->extra.geom_kind != 0;
    ri.manual_frames = h->manual_frames != 0; ri.normal_table = h->d_ntable != nullptr;
    ri.dyn_or_manual = h->dyn || ri.manual_frames || ri.normal_table;       // (manual_active is set in 6.)
    ri.use_gather = h->sw.kernel_gather; ri.item_run = h->d_item_run != nullptr; ri.frames_per_stage = h->frames_per_stage; ri.max_window = p.max_window;
    ri.bond_tiles = !p.tiles.empty(); ri.ua_tiles = !p.ua_tiles.empty(); ri.direct_items = !p.direct.empty(); ri.ua_fast_flag = (h->tables.flags & GORDER_FLAG_UA_FAST_NORMALISE) != 0;
    ri.global_leaflets = h->tables.leaflets.method == GORDER_LEAFLETS_GLOBAL; ri.spec_enabled = h->spec_enabled && !h->corr.on(); ri.have_assignment = h->have_assignment;
    ri.shells = h->n_shells != 0;
    ri.dist = h->hist_edges != 0;
    ri.classes = h->nb.on();
    ri.mol_rows = h->mol.n_groups != 0 && !h->mol_failed;
    ri.ua_samples_flag = (h->tables.flags & GORDER_FLAG_UA_SAMPLES) != 0;
    ri.npf5 = h->sw.npf5; ri.tw_gather = h->sw.tw_gather; ri.maps_gather = h->sw.maps_gather;
    ri.every_frame_assigns = b.aframes.size() == b.n_frames;
    b.route = gorder::choose_order_route(ri);
    if (!b.route.speculative) return;
    spec_poll(h, false);
    const uint32_t slot = (uint32_t)(h->spec_batches % gorder_hip_handle::kSpecRing);
    if (h->spec_ring_frames[slot]) (void)hipEventSynchronize(h->spec_counters_copied[slot]), spec_poll(h, false);
    ri.spec_enabled = h->spec_enabled && !h->corr.on();
    if (!ri.spec_enabled) b.route = gorder::choose_order_route(ri);      // the counters of an earlier batch turned it off
}

// 4. the flag rows: room for them, the frames' rows on the device, then the sides of the assignment frames (a speculative
// batch: after the order kernel, in 8.).  The first kernel of the batch is queued here or in 6.
static int fill_flag_rows(gorder_hip_handle *h, Batch &b) {
    if (!b.leaflets) return GORDER_OK;
    const bool spec = b.route.speculative;
    if (spec) std::fill(b.arow.begin(), b.arow.end(), 0u);
    const size_t rows = (b.ltable ? b.replay.expand.size() : b.aframes.size()) + 1;   // (a speculative batch: row 0 and every frame's exact sides)
    ST_TRY(ensure_flag_rows(h, rows, rows + rows / 4, true));
    ST_TRY(upload_if_changed(h, h->d_arow, h->up_arow, h->up_arow_valid, b.arow));
    if (h->collect & GORDER_COLLECT_LEAFLETS)
        for (uint32_t f : b.aframes) b.collect_frames.push_back(b.frame_index[f]);
    if (spec) b.spec_aframes = b.aframes;
    else if (b.ltable) BATCH_TRY(replay_flag_rows(h, b.replay));
    else BATCH_TRY(run_leaflets(h, b.d_xyz, b.d_box, b.aframes, 1));
    h->have_assignment = true;
    h->assignment_frame = b.last_assign_frame;
    b.n_new_rows = spec ? 0 : (b.ltable ? b.replay.expand.size() : b.aframes.size());
    return GORDER_OK;
}

// 5. grow the per-frame rows (timewise.rs:183-186).  A failure in here returns without abort_batch, as it always has.
static int grow_frame_rows(gorder_hip_handle *h, const Batch &b) {
    if (!h->extra.tw || h->n_frames + b.n_frames <= h->tw_cap) return GORDER_OK;
    const size_t row = 3 * (size_t)h->plan.n_acc;
    const uint64_t ncap = (h->n_frames + b.n_frames) * 2;
    DBuf<u64> ns, nc;      // (adopted once the copies are through)
    ST_TRY(allocate(h, ns, ncap * row));
    ST_TRY(allocate(h, nc, ncap * row));
    // everything on the handle's own (non-blocking) stream: a null-stream memset / copy is NOT ordered
    // with the kernels that follow and left stale rows behind (seen as a wrong error estimate)
    HIP_TRY(h, hipMemsetAsync(ns, 0, ncap * row * sizeof(u64), h->stream));
    HIP_TRY(h, hipMemsetAsync(nc, 0, ncap * row * sizeof(u64), h->stream));
    if (h->d_tw_sums) {
        HIP_TRY(h, hipMemcpyAsync(ns, h->d_tw_sums, h->n_frames * row * sizeof(u64), hipMemcpyDeviceToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(nc, h->d_tw_cnts, h->n_frames * row * sizeof(u64), hipMemcpyDeviceToDevice, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    h->d_tw_sums.swap(ns); h->d_tw_cnts.swap(nc); h->tw_cap = ncap;
    return GORDER_OK;
}

// 6. the kernels' common arguments, and the normals supplied for this batch: handed over for exactly these frames
// (gorder_hip_set_normals, checked in 1.) or the rows of the table, unpacked behind whatever still reads the buffer
static int set_batch_normals(gorder_hip_handle *h, Batch &b) {
    const Plan &p = h->plan;
    FrameArgs &a = b.a;
    a.xyz = b.d_xyz; a.box9 = b.d_box; a.n_atoms = p.n_atoms; a.n_frames = b.n_frames;
    a.pbc = b.pbc ? 1 : 0;
    a.nx = h->tables.normal[0]; a.ny = h->tables.normal[1]; a.nz = h->tables.normal[2]; a.n2 = h->n2; a.n2sq = h->n2sq;
    a.leaflets = b.leaflets ? 1 : 0; a.aflags = h->d_aflags; a.arow = h->d_arow; a.n_mol_total = p.n_mol_total;
    a.acc = h->d_acc; a.rep = h->d_rep; a.n_rep = h->sw.replicas; a.n_acc = p.n_acc; a.err = h->d_err;
    h->manual_active = false;
    if (h->manual_frames) {
        const size_t n4 = (size_t)b.n_frames * p.n_mol_total;
        BATCH_TRY(ensure(h, h->d_dyn_normals, n4));
        if (hipStreamSynchronize(h->stream) != hipSuccess ||   // earlier batches may still read the buffer
            hipMemcpy(h->d_dyn_normals, h->manual_normals.data(), n4 * 4 * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
            return b.abort_batch(h, fail(h, GORDER_ERR_DEVICE, "manual normals: copy to the device failed"));
        h->manual_active = true;
        h->manual_frames = 0;
    } else if (h->d_ntable) {
        BATCH_TRY(replay_normal_rows(h, b.normal_rows));
        h->manual_active = true;
    }
    return GORDER_OK;
}

// 7. the order kernels, with what a speculative batch and collected normals need them to write besides
static int run_batch_orders(gorder_hip_handle *h, Batch &b) {
    const Plan &p = h->plan;
    FrameArgs &a = b.a;
    if (b.route.speculative) {
        BATCH_TRY(ensure(h, h->d_mom, (size_t)b.n_frames * p.tiles.size()));
        BATCH_TRY(ensure(h, h->d_head_z, (size_t)b.n_frames * p.n_mol_total));
        a.own = h->d_own; a.mom = h->d_mom; a.mom_dim = (int)h->tables.leaflets.normal_dim;
        a.own_head_begin = h->d_own_head_begin; a.own_heads = h->d_own_heads; a.head_z = h->d_head_z;
    }
    h->extra.touched = nullptr;
    if ((h->collect & GORDER_COLLECT_NORMALS) && h->extra.geom_kind && !p.tiles.empty() && p.ua_tiles.empty()) {
        // bond systems fetch a molecule's normal after the geometry test (bond.rs:424-431): k_bonds_extras marks who did
        const size_t nt = (size_t)b.n_frames * p.n_mol_total;
        BATCH_TRY(ensure(h, h->d_touched, nt));
        if (hipMemsetAsync(h->d_touched, 0, nt, h->stream) != hipSuccess) return b.abort_batch(h, fail(h, GORDER_ERR_DEVICE, "collect: hipMemsetAsync"));
        h->extra.touched = h->d_touched;
    }
    h->mol_frame_index = b.frame_index;
    const int st = launch_orders(h, a, b.route);
    h->mol_frame_index = nullptr;
    h->manual_active = false;
    BATCH_TRY(st);
    h->rep_dirty = true;
    return GORDER_OK;
}

// 8. behind a speculative order kernel: the exact centres from its sums (k_spec_check), the exact kernel for the frames they
// cannot vouch for, the sides of every (frame, molecule) against the prediction, the mispredicted ones moved (k_spec_fixup)
static int resolve_speculation(gorder_hip_handle *h, Batch &b) {
    if (!b.route.speculative) return GORDER_OK;
    const Plan &p = h->plan;
    const gorder_leaflets_t &lf = h->tables.leaflets;
    const uint32_t n_frames = b.n_frames;
    BATCH_TRY(ensure(h, h->d_spec_center, n_frames));
    BATCH_TRY(ensure(h, h->d_spec_ok, n_frames));
    uint32_t *cnt = h->d_spec_counters + 2u * (uint32_t)(h->spec_batches & 1u);
    uint32_t *cnt_next = h->d_spec_counters + 2u * (uint32_t)((h->spec_batches + 1u) & 1u);
    SpecArgs sa{};
    sa.xyz = b.d_xyz; sa.box9 = b.d_box; sa.n_atoms = p.n_atoms; sa.n_frames = n_frames; sa.n_tiles = (uint32_t)p.tiles.size();
    sa.n_mol_total = p.n_mol_total; sa.n_membrane = lf.n_membrane; sa.dim = lf.normal_dim; sa.flip = lf.flip ? 1 : 0;
    sa.pbc = b.pbc ? 1 : 0; sa.mom = h->d_mom; sa.head_z = h->d_head_z; sa.center = h->d_spec_center; sa.ok = h->d_spec_ok;
    sa.aflags = h->d_aflags; sa.adist = h->d_adist; sa.counters = cnt; sa.counters_next = cnt_next;
    const uint32_t ring_slot = (uint32_t)(h->spec_batches % gorder_hip_handle::kSpecRing);
    sa.host_counters = h->h_spec_counters + 2u * ring_slot; sa.err = h->d_err;
    (void)timing_mark(h, "k_spec_check + k_spec_fixup");
    hipLaunchKernelGGL(k_spec_check, dim3(std::min<uint32_t>(n_frames, 2048u)), dim3(256), 0, h->stream, sa);
    BATCH_TRY(run_leaflets(h, b.d_xyz, b.d_box, b.spec_aframes, 1, h->d_spec_ok));
    (void)timing_mark(h, "k_spec_check + k_spec_fixup");
    const uint32_t fix_grid = (uint32_t)std::min<uint64_t>(((uint64_t)n_frames * p.n_mol_total + 63u) / 64u, 4096u);
    with_bool(b.route.fixup_ac, [&](auto AC) { with_bool(b.route.fixup_tw, [&](auto TW) {
        if constexpr (!AC() || !TW())      // (per-frame rows come out of the tiled kernel with the default cosine only)
            hipLaunchKernelGGL((k_spec_fixup<AC(), TW()>), dim3(fix_grid), dim3(64), 0, h->stream, b.a, sa, h->d_spec_mol_begin,
                               h->d_spec_samples, TW() ? h->d_tw_sums : nullptr, TW() ? h->d_tw_cnts : nullptr,
                               TW() ? (uint64_t)h->n_frames : (uint64_t)0);
    }); });
    hipLaunchKernelGGL(k_spec_finish, dim3(1), dim3(256), 0, h->stream, sa);
    HIP_TRY(h, hipGetLastError());      // (this exit and the next return without abort_batch, as they always have)
    HIP_TRY(h, hipEventRecord(h->spec_counters_copied[ring_slot], h->stream));
    h->spec_ring_frames[ring_slot] = n_frames;
    h->spec_batches++;
    return GORDER_OK;
}

// 10. the history a host asked for (rows 1.. of d_aflags hold every assignment frame's exact sides by now)
static int collect_batch(gorder_hip_handle *h, const Batch &b) {
    BATCH_TRY(collect_flag_rows(h, 1, b.collect_frames));
    if (b.ltable && (h->collect & GORDER_COLLECT_LEAFLETS)) {
        // a table: only the rows an assignment frame opened (a batch that starts inside an interval re-expands its row and
        // appends nothing, as priming does), in runs of consecutive rows
        const gorder::ReplayLeafletBatch &replay = b.replay;
        for (size_t k = 0; k < replay.collect_rows.size();) {
            size_t e = k + 1;
            while (e < replay.collect_rows.size() && replay.collect_rows[e] == replay.collect_rows[e - 1] + 1u) e++;
            const std::vector<uint64_t> run(replay.collect_frames.begin() + k, replay.collect_frames.begin() + e);
            BATCH_TRY(collect_flag_rows(h, replay.collect_rows[k], run));
            k = e;
        }
    }
    if ((h->collect & GORDER_COLLECT_NORMALS) && h->plan.n_mol_total && !h->d_ntable)
        BATCH_TRY(collect_normal_rows(h, b.frame_index, b.n_frames, h->extra.touched));
    return GORDER_OK;
}

// 11. what the next batch and a later error report find: the carry rows, the batch's frames under its ordinal, and — in one
// launch behind the batch's kernels — check_box, total_frames and the batch's error key (it becomes the run's unless an
// earlier batch had one).  No exit of this stage goes through abort_batch, as none ever has.
static int close_batch(gorder_hip_handle *h, const Batch &b) {
    const Plan &p = h->plan;
    const uint64_t *frame_index = b.frame_index;
    const uint32_t n_frames = b.n_frames;
    if (b.n_new_rows) {   // newest assignment becomes the carry row of the next batch (a failure returns without abort_batch)
        HIP_TRY(h, hipMemcpyAsync(h->d_aflags, h->d_aflags + b.n_new_rows * (size_t)p.n_mol_total, p.n_mol_total,
                                  hipMemcpyDeviceToDevice, h->stream));
    }
    if (b.ltable) { h->replay_have_carry = b.replay.have_carry; h->replay_carry_index = b.replay.carry_index; }
    gorder_hip_handle::BatchLog rec{h->n_submits, frame_index[0], n_frames > 1 ? frame_index[1] - frame_index[0] : 0, {}};
    for (uint32_t f = 1; f < n_frames; f++)
        if (frame_index[f] != rec.first + (uint64_t)f * rec.stride) { rec.list.assign(frame_index, frame_index + n_frames); break; }
    if (h->batch_log.size() >= gorder_hip_handle::kBatchLog) h->batch_log.pop_front();
    h->batch_log.push_back(std::move(rec));
    if (b.ri.mol_rows) {
        if (h->mol_batch_log.size() >= gorder_hip_handle::kBatchLog) h->mol_batch_log.pop_front();
        h->mol_batch_log.push_back({h->n_submits, b.mol_rows_before});
    }
    TIMING_MARK(h, "k_batch_end");        // (this exit and the two below return without abort_batch)
    hipLaunchKernelGGL(k_batch_end, dim3(b.pbc ? std::min<uint32_t>((n_frames + 255u) / 256u, 256u) : 1u), dim3(256), 0, h->stream,
                       b.pbc ? b.d_box : nullptr, n_frames, h->d_err,
                       h->d_acc + 4 * (size_t)p.n_acc, (unsigned long long)h->n_submits, h->decoder_key);
    HIP_TRY(h, hipGetLastError());
    TIMING_MARK(h, nullptr);          // the batch's chain of timed segments ends here
    if (h->timing_on) h->timing_launches++;
    h->n_submits++;
    h->n_frames += n_frames;
    if (h->corr.on()) h->corr.seen += n_frames;
    return GORDER_OK;
}

// One batch of frames, stage by stage (the numbers are those of the stages' comments above).  Up to the first kernel — the
// leaflet kernels of 4., or the table's normals in 6. — a failure simply returns; behind it, it leaves through
// Batch::abort_batch.  The exits that do not, although kernels are queued (growing the per-frame rows in 5., behind the
// speculation kernels in 8., the carry-row copy and k_batch_end in 11.), are kept as they were and say so where they stand:
// what a failed submit leaves behind is not this function's to change.
int gorder_hip_submit_device(gorder_hip_handle *h, const float *d_xyz, const float *d_box,
                             const uint64_t *frame_index, uint32_t n_frames) {
    if (!h || !d_xyz || !frame_index) return GORDER_ERR_INVALID_ARGUMENT;
    Batch b{d_xyz, d_box, frame_index, n_frames};
    b.pbc = h->tables.handle_pbc != 0;
    b.leaflets = h->tables.leaflets.method != GORDER_LEAFLETS_NONE;
    if (b.pbc && !d_box) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "box required when handle_pbc = 1");
    if (((uintptr_t)d_xyz & 15u) != 0) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "d_xyz must be 16-byte aligned");
    if (n_frames == 0) return GORDER_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    h->collect_locked = true;
    b.mol_rows_before = h->mol_store.n_rows();
    ST_TRY(check_batch(h, b));                  //  1. nothing is queued by 1. to 3.
    ST_TRY(plan_batch_rows(h, b));              //  2.
    choose_batch_route(h, b);                   //  3.
    ST_TRY(fill_flag_rows(h, b));               //  4.
    ST_TRY(grow_frame_rows(h, b));              //  5.
    ST_TRY(set_batch_normals(h, b));            //  6.
    ST_TRY(run_batch_orders(h, b));             //  7.
    ST_TRY(resolve_speculation(h, b));          //  8.
    // 9. bond reorientation: an additional pass over the batch, behind everything that writes the flag rows
    if (h->corr.on()) BATCH_TRY(launch_bond_corr(h, b.a));
    ST_TRY(collect_batch(h, b));                // 10.
    return close_batch(h, b);                   // 11.
}

int gorder_hip_submit_host(gorder_hip_handle *h, const float *xyz, const float *box, const uint64_t *frame_index,
                           uint32_t n_frames) {
    if (!h || !xyz || !frame_index) return GORDER_ERR_INVALID_ARGUMENT;
    if (n_frames == 0) return GORDER_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    int st;
    const size_t nx = (size_t)n_frames * h->plan.n_atoms * 3u, nb = (size_t)n_frames * 9u;
    if (!h->copy_stream) {
        HIP_TRY(h, h->copy_stream.create());
        for (int k = 0; k < 2; k++) {
            HIP_TRY(h, h->stage_copied[k].create());
            HIP_TRY(h, h->stage_computed[k].create());
        }
    }
    const int b = h->stage_next;
    h->stage_next ^= 1;
    // this buffer was last read by the kernels of two calls ago (normally long finished); the kernels of the
    // previous call keep running on the other buffer while this copy is in flight
    if (h->stage_used[b]) HIP_TRY(h, hipEventSynchronize(h->stage_computed[b]));
    if ((st = ensure(h, h->d_stage_xyz[b], nx)) != GORDER_OK) return st;
    HIP_TRY(h, hipMemcpyAsync(h->d_stage_xyz[b], xyz, nx * sizeof(float), hipMemcpyHostToDevice, h->copy_stream));
    if (box) {
        if ((st = ensure(h, h->d_stage_box[b], nb)) != GORDER_OK) return st;
        HIP_TRY(h, hipMemcpyAsync(h->d_stage_box[b], box, nb * sizeof(float), hipMemcpyHostToDevice, h->copy_stream));
    }
    HIP_TRY(h, hipEventRecord(h->stage_copied[b], h->copy_stream));
    HIP_TRY(h, hipStreamWaitEvent(h->stream, h->stage_copied[b], 0));
    st = gorder_hip_submit_device(h, h->d_stage_xyz[b], box ? h->d_stage_box[b] : nullptr, frame_index, n_frames);
    if (st != GORDER_OK) return st;
    HIP_TRY(h, hipEventRecord(h->stage_computed[b], h->stream));
    h->stage_used[b] = true;
    // the caller owns its buffer again when this returns
    HIP_TRY(h, hipEventSynchronize(h->stage_copied[b]));
    return GORDER_OK;
}

int gorder_hip_prime_leaflets(gorder_hip_handle *h, const float *d_xyz, const float *d_box, uint64_t frame_index) {
    if (!h || !d_xyz) return GORDER_ERR_INVALID_ARGUMENT;
    const gorder_leaflets_t &lf = h->tables.leaflets;
    if (lf.method == GORDER_LEAFLETS_NONE || lf.method == GORDER_LEAFLETS_MANUAL) return GORDER_ERR_INVALID_ARGUMENT;
    if (h->tables.handle_pbc && !d_box) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "box required when handle_pbc = 1");
    HIP_TRY(h, hipSetDevice(h->device));
    h->collect_locked = true;     // (no row: the primed frame belongs to the shard that analyses it)
    if (h->tables.handle_pbc) {   // the priming frame goes through check_box like any analysed frame (common.rs:186-198)
        hipLaunchKernelGGL(k_check_box, dim3(1), dim3(256), 0, h->stream, d_box, 1u, h->d_err);
        HIP_TRY(h, hipGetLastError());
    }
    ST_TRY(ensure_flag_rows(h, 2, 2, false));
    std::vector<uint32_t> aframes(1, 0);
    if (lf.method == GORDER_LEAFLETS_CLUSTERING) {
        if (frame_index != 0 && !h->cl_have_carry)
            return fail(h, GORDER_ERR_LEAFLETS_NOT_PRIMED, "clustering: prime frame 0 before a later assignment frame");
        h->cl_is0.assign(1, frame_index == 0 ? 1 : 0);
    }
    const int st = run_leaflets(h, d_xyz, d_box, aframes, 0);
    (void)timing_mark(h, nullptr);      // (the priming frame's kernels are a chain of their own: nothing stays open until the next submit)
    if (st != GORDER_OK) return st;
    h->have_assignment = true;
    h->assignment_frame = frame_index;
    return GORDER_OK;
}

int gorder_hip_set_manual_leaflets(gorder_hip_handle *h, const uint8_t *flags, uint64_t frame_index) {
    if (!h || !flags) return GORDER_ERR_INVALID_ARGUMENT;
    if (h->tables.leaflets.method != GORDER_LEAFLETS_MANUAL) return GORDER_ERR_INVALID_ARGUMENT;
    if (h->d_ltable) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_set_manual_leaflets: a manual leaflet table is set");
    HIP_TRY(h, hipSetDevice(h->device));
    const uint32_t n = h->plan.n_mol_total;
    std::vector<uint8_t> tmp(n);
    for (uint32_t i = 0; i < n; i++) tmp[i] = (uint8_t)((flags[i] & 1) ^ (h->tables.leaflets.flip ? 1 : 0));
    ST_TRY(ensure_flag_rows(h, 1, 2, false));      // (one row is read; the block is made with room for a batch's first)
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(h->d_aflags, tmp.data(), n, hipMemcpyHostToDevice));
    h->have_assignment = true;
    h->assignment_frame = frame_index;
    h->collect_locked = true;
    if (h->collect & GORDER_COLLECT_LEAFLETS) {     // the row the host handed over is an assignment frame's row like any other
        const int st = collect_flag_rows(h, 0, std::vector<uint64_t>(1, frame_index));
        (void)timing_mark(h, nullptr);
        if (st != GORDER_OK) return st;
    }
    return GORDER_OK;
}

int gorder_hip_synchronize(gorder_hip_handle *h) {
    if (!h) return GORDER_ERR_INVALID_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return check_device_error(h);
}

int gorder_hip_finish(gorder_hip_handle *h, int64_t *sums, uint64_t *counts, int64_t *map_sums,
                      uint64_t *map_counts, uint64_t *n_frames_analyzed) {
    if (!h) return GORDER_ERR_INVALID_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    int st = fold_replicas(h);
    if (st != GORDER_OK) return st;
    if ((st = fold_maps(h)) != GORDER_OK) return st;
    st = gorder_hip_synchronize(h);
    if (st != GORDER_OK) return st;
    const uint32_t n = h->plan.n_acc;
    std::vector<unsigned long long> raw(4 * (size_t)n + 1);
    HIP_TRY(h, hipMemcpy(raw.data(), h->d_acc, raw.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    const bool lf = h->tables.leaflets.method != GORDER_LEAFLETS_NONE;
    for (uint32_t s = 0; s < n; s++) {
        const int64_t tot = (int64_t)raw[s], up = (int64_t)raw[n + s];
        const uint64_t ctot = raw[2 * (size_t)n + s], cup = raw[3 * (size_t)n + s];
        if (sums) {
            sums[s] = tot;
            sums[n + s] = lf ? up : 0;
            sums[2 * (size_t)n + s] = lf ? tot - up : 0;   // every sample is upper or lower (bond.rs:199-213)
        }
        if (counts) {
            counts[s] = ctot;
            counts[n + s] = lf ? cup : 0;
            counts[2 * (size_t)n + s] = lf ? ctot - cup : 0;
        }
    }
    if (n_frames_analyzed) *n_frames_analyzed = raw[4 * (size_t)n];
    if (h->extra.maps) {
        const size_t nmap = 3 * (size_t)n * h->map_nx * h->map_ny;
        if (map_sums) HIP_TRY(h, hipMemcpy(map_sums, h->d_map_sums, nmap * sizeof(int64_t), hipMemcpyDeviceToHost));
        if (map_counts) HIP_TRY(h, hipMemcpy(map_counts, h->d_map_cnts, nmap * sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
    return GORDER_OK;
}

int gorder_hip_set_normals(gorder_hip_handle *h, const float *normals, uint32_t n_frames) {
    if (!h || !normals || n_frames == 0) return GORDER_ERR_INVALID_ARGUMENT;
    if (h->d_ntable) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_set_normals: a manual normal table is set");
    if (h->n_shells) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_set_normals: the handle has radial shells (static normals only)");
    if (h->mol.n_groups) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_set_normals: the handle has molecule rows (static normals only)");
    if (h->hist_edges) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_set_normals: the handle has an order histogram (static normals only)");
    if (h->nb.on()) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_set_normals: the handle has neighbour classes (static normals only)");
    const size_t n = (size_t)n_frames * h->plan.n_mol_total;
    h->manual_normals.resize(4 * n);
    for (size_t i = 0; i < n; i++) {
        h->manual_normals[4 * i + 0] = normals[3 * i + 0];
        h->manual_normals[4 * i + 1] = normals[3 * i + 1];
        h->manual_normals[4 * i + 2] = normals[3 * i + 2];
        h->manual_normals[4 * i + 3] = 3.0f;     // "enough points": the sample kernels treat it like a computed normal
    }
    h->manual_frames = n_frames;
    return GORDER_OK;
}

// ---- whole-trajectory manual tables ---------------------------------------------------------------------------------------
// The only calls of the replay that wait: the new table is allocated and filled first (a failure leaves the old one in
// place), then the stream is drained, since batches still queued may read the old table, and the old table is freed.
int gorder_hip_set_manual_leaflet_table(gorder_hip_handle *h, const uint8_t *flags, uint64_t first_row, uint64_t n_rows) {
    if (!h || (n_rows && !flags)) return GORDER_ERR_INVALID_ARGUMENT;
    if (h->tables.leaflets.method != GORDER_LEAFLETS_MANUAL)
        return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_set_manual_leaflet_table: leaflets.method is not GORDER_LEAFLETS_MANUAL");
    const uint32_t n_mol = h->plan.n_mol_total;
    if (n_rows && (!n_mol || !gorder::replay_window_ok(first_row, n_rows)))
        return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_set_manual_leaflet_table: no molecules, or more than 2^32 - 1 rows");
    HIP_TRY(h, hipSetDevice(h->device));
    DBuf<u64> nt;
    if (n_rows) {
        const size_t wpr = gorder::replay_flag_words(n_mol);
        std::vector<uint64_t> words((size_t)n_rows * wpr);
        for (uint64_t r = 0; r < n_rows; r++) gorder::replay_pack_flags(flags + r * (size_t)n_mol, n_mol, words.data() + r * wpr);
        if (!nt.alloc(words.size())) {
            (void)hipGetLastError();         // (the handle stays usable: the error is reported here, not by the next launch)
            return fail(h, GORDER_ERR_DEVICE, "gorder_hip_set_manual_leaflet_table: hipMalloc failed");
        }
        if (hipMemcpy(nt, words.data(), words.size() * sizeof(uint64_t), hipMemcpyHostToDevice) != hipSuccess)
            return fail(h, GORDER_ERR_DEVICE, "gorder_hip_set_manual_leaflet_table: copy to the device failed");
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->d_ltable = std::move(nt);
    h->ltable_win.first_row = n_rows ? first_row : 0;
    h->ltable_win.n_rows = n_rows;
    // the row carried so far belongs to whatever supplied it: the next batch takes its first row from the new source
    h->replay_have_carry = false;
    h->have_assignment = false;
    return GORDER_OK;
}

int gorder_hip_set_manual_normal_table(gorder_hip_handle *h, const float *normals, uint32_t step, uint64_t first_row, uint64_t n_rows) {
    if (!h || (n_rows && !normals)) return GORDER_ERR_INVALID_ARGUMENT;
    if (h->n_shells) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_set_manual_normal_table: the handle has radial shells (static normals only)");
    if (h->mol.n_groups) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_set_manual_normal_table: the handle has molecule rows (static normals only)");
    if (h->hist_edges) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_set_manual_normal_table: the handle has an order histogram (static normals only)");
    if (h->nb.on()) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_set_manual_normal_table: the handle has neighbour classes (static normals only)");
    const uint32_t n_mol = h->plan.n_mol_total;
    if (n_rows) {
        if (step == 0) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_set_manual_normal_table: step 0");
        if (!n_mol || !gorder::replay_window_ok(first_row, n_rows))
            return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_set_manual_normal_table: no molecules, or more than 2^32 - 1 rows");
        if (!h->plan.direct.empty()) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "manual normals: a bond spans more than the LDS window");
    }
    HIP_TRY(h, hipSetDevice(h->device));
    DBuf<ReplayVec3> nt;
    if (n_rows) {
        const size_t n = (size_t)n_rows * n_mol;
        if (!nt.alloc(n)) {
            (void)hipGetLastError();
            return fail(h, GORDER_ERR_DEVICE, "gorder_hip_set_manual_normal_table: hipMalloc failed");
        }
        if (hipMemcpy(nt, normals, n * sizeof(ReplayVec3), hipMemcpyHostToDevice) != hipSuccess)
            return fail(h, GORDER_ERR_DEVICE, "gorder_hip_set_manual_normal_table: copy to the device failed");
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->d_ntable = std::move(nt);
    h->ntable_win.first_row = n_rows ? first_row : 0;
    h->ntable_win.n_rows = n_rows;
    h->ntable_step = n_rows ? step : 1;
    h->manual_frames = 0;                    // normals handed over for "the next submit" give way to the table
    return GORDER_OK;
}

int gorder_hip_normals(gorder_hip_handle *h, float *normals, uint32_t *n_points) {
    if (!h || !h->dyn) return GORDER_ERR_INVALID_ARGUMENT;
    ST_TRY(gorder_hip_synchronize(h));
    const uint32_t n_mol = h->plan.n_mol_total;
    if (h->last_normals.size() < 4 * (size_t)n_mol) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "no frame submitted yet");
    for (uint32_t m = 0; m < n_mol; m++) {
        if (normals) for (int d = 0; d < 3; d++) normals[3 * (size_t)m + d] = h->last_normals[4 * (size_t)m + d];
        if (n_points) n_points[m] = (uint32_t)h->last_normals[4 * (size_t)m + 3];
    }
    return GORDER_OK;
}

int gorder_hip_timewise(gorder_hip_handle *h, int64_t *tw_sums, uint64_t *tw_counts, uint64_t capacity_frames) {
    if (!h || !h->extra.tw || !tw_sums || !tw_counts) return GORDER_ERR_INVALID_ARGUMENT;
    if (capacity_frames < h->n_frames) return GORDER_ERR_INVALID_ARGUMENT;
    ST_TRY(gorder_hip_synchronize(h));
    const size_t n = h->n_frames * 3 * (size_t)h->plan.n_acc;
    if (n) {
        HIP_TRY(h, hipMemcpy(tw_sums, h->d_tw_sums, n * sizeof(int64_t), hipMemcpyDeviceToHost));
        HIP_TRY(h, hipMemcpy(tw_counts, h->d_tw_cnts, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
        // the kernels keep total and upper only (a third fewer atomics): the lower leaflet's rows are their difference
        if (h->tables.leaflets.method != GORDER_LEAFLETS_NONE) {
            const size_t na = h->plan.n_acc;
            for (uint64_t f = 0; f < h->n_frames; f++) {
                int64_t *s = tw_sums + f * 3 * na;
                uint64_t *c = tw_counts + f * 3 * na;
                for (size_t k = 0; k < na; k++) { s[2 * na + k] = s[k] - s[na + k]; c[2 * na + k] = c[k] - c[na + k]; }
            }
        }
    }
    return GORDER_OK;
}

// ---- error estimates and convergence from the rows, on the device (kernels_timewise.h, timewise_blocks.h) ---------------
uint32_t gorder_hip_timewise_chunk_frames(void) { return gorder::kTwChunkFrames; }

uint64_t gorder_hip_timewise_rows(const gorder_hip_handle *h) { return h && h->extra.tw ? h->n_frames : 0; }

// what every entry point below refuses, and the wait for the rows (a device error of the run is returned as by gorder_hip_synchronize)
static int tw_enter(gorder_hip_handle *h, const char *who, uint32_t n_blocks) {
    if (!h) return GORDER_ERR_INVALID_ARGUMENT;
    if (!h->extra.tw) return fail(h, GORDER_ERR_INVALID_ARGUMENT, std::string(who) + ": the handle keeps no per-frame rows (tables.timewise = 0)");
    if (n_blocks < 2) return fail(h, GORDER_ERR_INVALID_ARGUMENT, std::string(who) + ": n_blocks must be at least 2");
    return gorder_hip_synchronize(h);
}

// the groups, checked and copied to d_twx_groups: group_begin rebased to 0 [n_groups + 1], then the slots
static int tw_upload_groups(gorder_hip_handle *h, const char *who, const uint32_t *group_begin, const uint32_t *slots, uint32_t n_groups) {
    uint32_t bad = 0;
    const gorder::TwGroupStatus gs = gorder::tw_check_groups(group_begin, slots, n_groups, h->plan.n_acc, &bad);
    if (gs != gorder::kTwGroupsOk)
        return fail(h, GORDER_ERR_INVALID_ARGUMENT, std::string(who) + ": " + gorder::tw_group_status_text(gs) + " (at " + std::to_string(bad) + ")");
    std::vector<uint32_t> csr((size_t)n_groups + 1u);
    for (uint32_t g = 0; g <= n_groups; g++) csr[g] = group_begin[g] - group_begin[0];
    csr.insert(csr.end(), slots + group_begin[0], slots + group_begin[n_groups]);
    ST_TRY(ensure(h, h->d_twx_groups, csr.size()));
    HIP_TRY(h, hipMemcpyAsync(h->d_twx_groups, csr.data(), csr.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));      // (csr leaves scope)
    return GORDER_OK;
}

// d_twx_blocks = the block sums [n_blocks][3][n_acc], then the counts, of this handle's rows; queued on the stream
static int tw_blocks_device(gorder_hip_handle *h, uint32_t n_blocks, uint64_t total_frames, uint64_t first_position, uint64_t *block_size) {
    const uint32_t n_acc = h->plan.n_acc, row_words = 3u * n_acc;
    const bool leaflets = h->tables.leaflets.method != GORDER_LEAFLETS_NONE;
    if (!gorder::tw_positions_ok(first_position, h->n_frames))
        return fail(h, GORDER_ERR_INVALID_ARGUMENT, "first_position + the handle's rows passes 2^64");
    const uint64_t bs = gorder::tw_block_size(total_frames, n_blocks);
    if (block_size) *block_size = bs;
    const size_t n = (size_t)n_blocks * row_words;
    int st = ensure(h, h->d_twx_blocks, 2 * n);
    if (st != GORDER_OK) return st;
    unsigned long long *d_sums = h->d_twx_blocks, *d_cnts = h->d_twx_blocks + n;
    HIP_TRY(h, hipMemsetAsync(h->d_twx_blocks, 0, 2 * n * sizeof(unsigned long long), h->stream));
    const uint64_t n_used = gorder::tw_rows_used(first_position, h->n_frames, bs, n_blocks);
    if (n_used == 0) return GORDER_OK;
    TIMING_MARK(h, "k_tw_blocks");
    const uint32_t fold_words = leaflets ? 2u * n_acc : row_words;
    const uint32_t threads = fold_words <= 64u ? 64u : (fold_words <= 128u ? 128u : 256u);
    hipLaunchKernelGGL(k_tw_blocks, dim3((uint32_t)gorder::tw_n_chunks(n_used), (fold_words + threads - 1u) / threads), dim3(threads), 0,
                       h->stream, h->d_tw_sums, h->d_tw_cnts, row_words, fold_words, (tw_u64)n_used, (tw_u64)first_position, (tw_u64)bs,
                       d_sums, d_cnts);
    HIP_TRY(h, hipGetLastError());
    if (leaflets) {
        const uint64_t m = (uint64_t)n_blocks * n_acc;
        hipLaunchKernelGGL(k_tw_lower, dim3((uint32_t)((m + 255u) / 256u)), dim3(256), 0, h->stream, d_sums, d_cnts, n_acc, (tw_u64)m);
        HIP_TRY(h, hipGetLastError());
    }
    TIMING_MARK(h, nullptr);
    return GORDER_OK;
}

int gorder_hip_timewise_blocks(gorder_hip_handle *h, uint32_t n_blocks, uint64_t total_frames, uint64_t first_position,
                               int64_t *block_sums, uint64_t *block_counts, uint64_t *block_size) {
    int st = tw_enter(h, "gorder_hip_timewise_blocks", n_blocks);
    if (st != GORDER_OK) return st;
    if (!block_sums || !block_counts) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_timewise_blocks: null output");
    if ((st = tw_blocks_device(h, n_blocks, total_frames, first_position, block_size)) != GORDER_OK) return st;
    const size_t n = (size_t)n_blocks * 3u * h->plan.n_acc;
    HIP_TRY(h, hipMemcpyAsync(block_sums, h->d_twx_blocks, n * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(block_counts, h->d_twx_blocks + n, n * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return GORDER_OK;
}

int gorder_hip_error_estimate(gorder_hip_handle *h, uint32_t n_blocks, const uint32_t *group_begin, const uint32_t *slots,
                              uint32_t n_groups, const int64_t *block_sums, const uint64_t *block_counts, float *errors) {
    int st = tw_enter(h, "gorder_hip_error_estimate", n_blocks);
    if (st != GORDER_OK) return st;
    if (!errors || (block_sums == nullptr) != (block_counts == nullptr))
        return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_error_estimate: null output, or only one of block_sums / block_counts");
    if ((st = tw_upload_groups(h, "gorder_hip_error_estimate", group_begin, slots, n_groups)) != GORDER_OK) return st;
    const uint32_t n_acc = h->plan.n_acc;
    const size_t n = (size_t)n_blocks * 3u * n_acc;
    if (block_sums) {            // merged blocks of several shards
        if ((st = ensure(h, h->d_twx_blocks, 2 * n)) != GORDER_OK) return st;
        HIP_TRY(h, hipMemcpyAsync(h->d_twx_blocks, block_sums, n * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(h->d_twx_blocks + n, block_counts, n * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
    } else if ((st = tw_blocks_device(h, n_blocks, h->n_frames, 0, nullptr)) != GORDER_OK) return st;
    if ((st = ensure(h, h->d_twx_out, (size_t)n_groups * 3u)) != GORDER_OK) return st;
    TIMING_MARK(h, "k_tw_errors");
    hipLaunchKernelGGL(k_tw_errors, dim3(n_groups * 3u), dim3(64), 0, h->stream, h->d_twx_blocks, h->d_twx_blocks + n, n_blocks, n_acc,
                       h->d_twx_groups, h->d_twx_groups + n_groups + 1u, h->d_twx_out);
    HIP_TRY(h, hipGetLastError());
    TIMING_MARK(h, nullptr);
    HIP_TRY(h, hipMemcpyAsync(errors, h->d_twx_out, (size_t)n_groups * 3u * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return GORDER_OK;
}

int gorder_hip_convergence(gorder_hip_handle *h, const uint32_t *group_begin, const uint32_t *slots, uint32_t n_groups,
                           const int64_t *carry_sums, const uint64_t *carry_counts, float *prefix, int64_t *end_sums,
                           uint64_t *end_counts) {
    int st = tw_enter(h, "gorder_hip_convergence", 2);
    if (st != GORDER_OK) return st;
    if ((carry_sums == nullptr) != (carry_counts == nullptr))
        return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_convergence: only one of carry_sums / carry_counts");
    if ((st = tw_upload_groups(h, "gorder_hip_convergence", group_begin, slots, n_groups)) != GORDER_OK) return st;
    const uint64_t n_frames = h->n_frames;
    const uint32_t n_cols = 3u * n_groups;
    if (n_frames == 0) {         // nothing to scan: the carry passes through
        for (uint32_t k = 0; k < n_cols; k++) {
            if (end_sums) end_sums[k] = carry_sums ? carry_sums[k] : 0;
            if (end_counts) end_counts[k] = carry_counts ? carry_counts[k] : 0;
        }
        return GORDER_OK;
    }
    if (!prefix) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_convergence: null output");
    const uint64_t n_chunks = gorder::tw_n_chunks(n_frames);
    const size_t n_rows = (size_t)n_frames * n_cols, n_tot = (size_t)n_chunks * n_cols;
    if ((st = ensure(h, h->d_twx_rows, 2 * n_rows)) != GORDER_OK) return st;
    if ((st = ensure(h, h->d_twx_totals, 2 * n_tot)) != GORDER_OK) return st;
    if ((st = ensure(h, h->d_twx_edge, 4 * (size_t)n_cols)) != GORDER_OK) return st;
    if ((st = ensure(h, h->d_twx_out, n_rows)) != GORDER_OK) return st;
    unsigned long long *d_rs = h->d_twx_rows, *d_rc = d_rs + n_rows, *d_ts = h->d_twx_totals, *d_tc = d_ts + n_tot;
    unsigned long long *d_cs = nullptr, *d_cc = nullptr, *d_es = h->d_twx_edge + 2 * (size_t)n_cols, *d_ec = d_es + n_cols;
    if (carry_sums) {
        d_cs = h->d_twx_edge; d_cc = d_cs + n_cols;
        HIP_TRY(h, hipMemcpyAsync(d_cs, carry_sums, n_cols * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(d_cc, carry_counts, n_cols * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
    }
    const uint32_t *d_begin = h->d_twx_groups, *d_slots = h->d_twx_groups + n_groups + 1u;
    const uint64_t n_waves = n_frames * n_groups;
    if ((n_waves + 3u) / 4u > 0x7fffffffull || (n_tot + 255u) / 256u > 0x7fffffffull)
        return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_convergence: more (frame, group) pairs than one launch takes");
    TIMING_MARK(h, "k_tw_group_rows");
    hipLaunchKernelGGL(k_tw_group_rows, dim3((uint32_t)((n_waves + 3u) / 4u)), dim3(256), 0, h->stream, h->d_tw_sums, h->d_tw_cnts,
                       h->plan.n_acc, h->tables.leaflets.method != GORDER_LEAFLETS_NONE ? 1 : 0, (tw_u64)n_frames, n_groups, d_begin, d_slots,
                       d_rs, d_rc);
    HIP_TRY(h, hipGetLastError());
    TIMING_MARK(h, "k_tw_chunk_totals + k_tw_scan_totals + k_tw_apply");
    const dim3 per_chunk((uint32_t)((n_tot + 255u) / 256u));
    hipLaunchKernelGGL(k_tw_chunk_totals, per_chunk, dim3(256), 0, h->stream, d_rs, d_rc, (tw_u64)n_frames, n_cols, (tw_u64)n_tot, d_ts, d_tc);
    HIP_TRY(h, hipGetLastError());
    hipLaunchKernelGGL(k_tw_scan_totals, dim3(n_cols), dim3(256), 0, h->stream, d_ts, d_tc, (tw_u64)n_chunks, n_cols, d_cs, d_cc, d_es, d_ec);
    HIP_TRY(h, hipGetLastError());
    hipLaunchKernelGGL(k_tw_apply, per_chunk, dim3(256), 0, h->stream, d_rs, d_rc, d_ts, d_tc, (tw_u64)n_frames, n_cols, (tw_u64)n_tot,
                       h->d_twx_out);
    HIP_TRY(h, hipGetLastError());
    TIMING_MARK(h, nullptr);
    HIP_TRY(h, hipMemcpyAsync(prefix, h->d_twx_out, n_rows * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (end_sums) HIP_TRY(h, hipMemcpyAsync(end_sums, d_es, n_cols * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    if (end_counts) HIP_TRY(h, hipMemcpyAsync(end_counts, d_ec, n_cols * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return GORDER_OK;
}

// ---- ordermaps finished on the device (kernels_ordermap.h, ordermap_final.h) ---------------------------------------------
int gorder_hip_ordermaps(gorder_hip_handle *h, const uint32_t *group_begin, const uint32_t *slots, uint32_t n_groups,
                         uint32_t min_samples, uint32_t negate, const void *d_sums, const void *d_counts, uint64_t n_u64, float *maps) {
    if (!h) return GORDER_ERR_INVALID_ARGUMENT;
    const std::string who = "gorder_hip_ordermaps: ";
    if (!h->extra.maps) return fail(h, GORDER_ERR_INVALID_ARGUMENT, who + "the handle keeps no ordermaps (tables.ordermap.enabled = 0)");
    if (!maps) return fail(h, GORDER_ERR_INVALID_ARGUMENT, who + "null output");
    if ((d_sums == nullptr) != (d_counts == nullptr)) return fail(h, GORDER_ERR_INVALID_ARGUMENT, who + "only one of d_sums / d_counts");
    const uint32_t n_acc = h->plan.n_acc;
    gorder::TwGroupStatus gs = gorder::kTwGroupsOk;
    uint32_t bad = 0;
    const gorder::OmStatus os = gorder::om_check(group_begin, slots, n_groups, n_acc, min_samples, &gs, &bad);
    if (os == gorder::kOmMinSamples) return fail(h, GORDER_ERR_INVALID_ARGUMENT, who + "min_samples must be at least 1");
    if (os != gorder::kOmOk)
        return fail(h, GORDER_ERR_INVALID_ARGUMENT, who + gorder::tw_group_status_text(gs) + " (at " + std::to_string(bad) + ")");
    const uint64_t n_tiles = (uint64_t)h->map_nx * h->map_ny, n_words = gorder::om_map_words(n_acc, h->map_nx, h->map_ny);
    if (d_sums && n_u64 != n_words)
        return fail(h, GORDER_ERR_INVALID_ARGUMENT, who + "n_u64 is " + std::to_string(n_u64) + ", the maps hold " + std::to_string(n_words) + " words");
    const uint64_t tile_blocks = (n_tiles + 255u) / 256u, n_blocks = (uint64_t)n_groups * 3u * tile_blocks;
    if (n_blocks > 0x7fffffffull) return fail(h, GORDER_ERR_INVALID_ARGUMENT, who + "more (group, tile) pairs than one launch takes");
    HIP_TRY(h, hipSetDevice(h->device));
    int st = fold_maps(h);
    if (st != GORDER_OK) return st;
    if ((st = gorder_hip_synchronize(h)) != GORDER_OK) return st;        // a device error of the run is returned here
    std::vector<uint32_t> csr((size_t)n_groups + 1u);
    for (uint32_t g = 0; g <= n_groups; g++) csr[g] = group_begin[g] - group_begin[0];
    csr.insert(csr.end(), slots + group_begin[0], slots + group_begin[n_groups]);
    if ((st = ensure(h, h->d_omx_groups, csr.size())) != GORDER_OK) return st;
    const size_t n_out = (size_t)n_groups * 3u * n_tiles;
    if ((st = ensure(h, h->d_omx_out, n_out)) != GORDER_OK) return st;
    HIP_TRY(h, hipMemcpyAsync(h->d_omx_groups, csr.data(), csr.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    TIMING_MARK(h, "k_map_finalise");
    hipLaunchKernelGGL(k_map_finalise, dim3((uint32_t)n_blocks), dim3(256), 0, h->stream,
                       d_sums ? (const om_u64 *)d_sums : h->d_map_sums, d_counts ? (const om_u64 *)d_counts : h->d_map_cnts, n_acc,
                       (om_u64)n_tiles, (uint32_t)tile_blocks, h->tables.leaflets.method != GORDER_LEAFLETS_NONE ? 3u : 1u,
                       h->d_omx_groups, h->d_omx_groups + n_groups + 1u, min_samples, negate ? 1 : 0, h->d_omx_out);
    HIP_TRY(h, hipGetLastError());
    TIMING_MARK(h, nullptr);
    HIP_TRY(h, hipMemcpyAsync(maps, h->d_omx_out, n_out * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));      // (csr leaves scope)
    return GORDER_OK;
}

int gorder_hip_leaflets(gorder_hip_handle *h, uint8_t *flags, uint64_t *assignment_frame) {
    if (!h) return GORDER_ERR_INVALID_ARGUMENT;
    if (!h->have_assignment) return GORDER_ERR_LEAFLETS_NOT_PRIMED;
    ST_TRY(gorder_hip_synchronize(h));
    if (flags) HIP_TRY(h, hipMemcpy(flags, h->d_aflags, h->plan.n_mol_total, hipMemcpyDeviceToHost));
    if (assignment_frame) *assignment_frame = h->assignment_frame;
    return GORDER_OK;
}

// ---- collected history: every assignment frame's flags, every analysed frame's dynamic normals --------------------------
int gorder_hip_set_collect(gorder_hip_handle *h, uint32_t what) {
    if (!h) return GORDER_ERR_INVALID_ARGUMENT;
    if (what & ~(uint32_t)(GORDER_COLLECT_LEAFLETS | GORDER_COLLECT_NORMALS)) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_set_collect: unknown bit");
    if (h->collect_locked)
        return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_set_collect: only before the first submit or prime, or right after gorder_hip_reset");
    if ((what & GORDER_COLLECT_LEAFLETS) && h->tables.leaflets.method == GORDER_LEAFLETS_NONE)
        return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_set_collect: no leaflet method to collect from");
    if ((what & GORDER_COLLECT_NORMALS) && !h->dyn)
        return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_set_collect: normals are collected for dynamic membrane normals only");
    if (what && !h->plan.n_mol_total) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_set_collect: no molecules");
    HIP_TRY(h, hipSetDevice(h->device));
    const gorder::CollectAlloc pinned{PinnedMem::alloc, PinnedMem::release};
    if ((what & GORDER_COLLECT_LEAFLETS) && !h->collect_flags.configured())
        h->collect_flags.configure(gorder::collect_flag_words(h->plan.n_mol_total) * sizeof(uint64_t), pinned);
    if ((what & GORDER_COLLECT_NORMALS) && !h->collect_normals.configured())
        h->collect_normals.configure((size_t)h->plan.n_mol_total * 3u * sizeof(float), pinned);
    h->collect_flags.clear();
    h->collect_normals.clear();
    h->collect = what;
    return GORDER_OK;
}

// ---- radial shells (kernels_radial.h) -----------------------------------------------------------------------------------
int gorder_hip_radial_thresholds(const float *radii, uint32_t n, float *thr) {
    if ((n && !radii) || (n && !thr)) return GORDER_ERR_INVALID_ARGUMENT;
    for (uint32_t k = 0; k < n; k++) thr[k] = local_radius_threshold(radii[k]);
    return GORDER_OK;
}

int gorder_hip_set_radial_shells(gorder_hip_handle *h, const float *radii, uint32_t n_radii) {
    if (!h || (n_radii && !radii)) return GORDER_ERR_INVALID_ARGUMENT;
    const char *who = "gorder_hip_set_radial_shells: ";
    auto refuse = [&](const char *why) { return fail(h, GORDER_ERR_INVALID_ARGUMENT, std::string(who) + why); };
    if (h->collect_locked) return refuse("only before the first submit or prime, or right after gorder_hip_reset");
    const Plan &p = h->plan;
    if (n_radii) {
        const gorder_tables_t &t = h->tables;
        if (h->mol.n_groups) return refuse("the handle has molecule rows");
        if (h->hist_edges) return refuse("the handle has an order histogram");
        if (h->nb.on()) return refuse("the handle has neighbour classes");
        if (n_radii > GORDER_RADIAL_MAX_SHELLS) return refuse("more than GORDER_RADIAL_MAX_SHELLS radii");
        if (t.geometry.kind != GORDER_GEOM_CYLINDER && t.geometry.kind != GORDER_GEOM_SPHERE)
            return refuse("the tables select no cylinder or sphere");
        if (t.geometry.invert) return refuse("the selection is inverted");
        if (!p.ua_tiles.empty()) return refuse("united-atom molecule types");
        if (h->extra.maps) return refuse("ordermaps are on");
        if (h->extra.tw) return refuse("timewise is on");
        if (h->dyn) return refuse("dynamic membrane normals");
        if (h->d_ntable) return refuse("a manual normal table is set");
        if (h->manual_frames) return refuse("normals were supplied by gorder_hip_set_normals");
        // (GORDER_COLLECT_NORMALS needs dynamic normals, gorder_hip_set_collect: refused above with them)
        if (!p.n_acc || p.tiles.empty()) return refuse("no bond samples");
        float thr[GORDER_RADIAL_MAX_SHELLS];
        for (uint32_t k = 0; k < n_radii; k++) {
            if (!std::isfinite(radii[k]) || !(radii[k] > 0.0f)) return refuse("a radius is not finite and > 0");
            if (k && !(radii[k] > radii[k - 1])) return refuse("the radii are not strictly ascending");
            thr[k] = local_radius_threshold(radii[k]);
            if (k && thr[k] < thr[k - 1]) return refuse("the radii's thresholds do not ascend");       // (sqrt is monotonic: never)
        }
        if (memcmp(&radii[n_radii - 1], &t.geometry.radius, sizeof(float)) != 0 || thr[n_radii - 1] != h->extra.geom_thr)
            return refuse("the last radius is not tables.geometry.radius");
        HIP_TRY(h, hipSetDevice(h->device));
        HIP_TRY(h, hipStreamSynchronize(h->stream));       // (a reset still queued may be zeroing the old blocks)
        h->n_shells = 0;
        // replicas against contention on the global shell words, as the ordinary sums have them (gorder::replica_count)
        ST_TRY(alloc_zeroed(h, h->shells, (size_t)n_radii * 4u * p.n_acc));
        uint32_t max_slots = 1;
        for (const Tile &tile : p.tiles) max_slots = std::max(max_slots, tile.n_slots);
        const uint32_t planes = t.leaflets.method != GORDER_LEAFLETS_NONE ? 2u : 1u;
        h->shell_lds_bytes = (size_t)planes * n_radii * max_slots * sizeof(unsigned long long);
        h->shell_direct = h->sw.radial_direct || h->shell_lds_bytes > 64u * 1024u;
        for (uint32_t k = 0; k < n_radii; k++) h->shell_thr[k] = thr[k];
        h->n_shells = n_radii;
        return GORDER_OK;
    }
    if (h->n_shells) {
        HIP_TRY(h, hipSetDevice(h->device));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        h->shells.reset();
        h->n_shells = 0;
    }
    return GORDER_OK;
}

int gorder_hip_radial_shells(gorder_hip_handle *h, int64_t *sums, uint64_t *counts, uint32_t *n_shells) {
    if (!h) return GORDER_ERR_INVALID_ARGUMENT;
    if (n_shells) *n_shells = h->n_shells;
    if (!h->n_shells) return GORDER_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const uint32_t n = h->plan.n_acc;
    HIP_TRY(h, h->shells.fold(h->stream));
    ST_TRY(gorder_hip_synchronize(h));
    std::vector<unsigned long long> raw(h->shells.words);
    HIP_TRY(h, hipMemcpy(raw.data(), h->shells.acc, raw.size() * sizeof(u64), hipMemcpyDeviceToHost));
    const bool lf = h->tables.leaflets.method != GORDER_LEAFLETS_NONE;
    for (uint32_t k = 0; k < h->n_shells; k++) {
        const unsigned long long *r = raw.data() + (size_t)k * 4u * n;
        for (uint32_t s = 0; s < n; s++) {
            const int64_t tot = (int64_t)r[s], up = (int64_t)r[n + s];
            const uint64_t ctot = r[2 * (size_t)n + s], cup = r[3 * (size_t)n + s];
            const size_t o = (size_t)k * 3u * n + s;
            if (sums) { sums[o] = tot; sums[o + n] = lf ? up : 0; sums[o + 2 * (size_t)n] = lf ? tot - up : 0; }
            if (counts) { counts[o] = ctot; counts[o + n] = lf ? cup : 0; counts[o + 2 * (size_t)n] = lf ? ctot - cup : 0; }
        }
    }
    return GORDER_OK;
}

// ---- order distributions (order_hist.h, kernels_hist.h) ------------------------------------------------------------------
int gorder_hip_set_order_histogram(gorder_hip_handle *h, const int32_t *edges, uint32_t n_edges) {
    if (!h || (n_edges && !edges)) return GORDER_ERR_INVALID_ARGUMENT;
    const char *who = "gorder_hip_set_order_histogram: ";
    auto refuse = [&](const char *why) { return fail(h, GORDER_ERR_INVALID_ARGUMENT, std::string(who) + why); };
    if (h->collect_locked) return refuse("only before the first submit or prime, or right after gorder_hip_reset");
    const Plan &p = h->plan;
    const bool ua_samples = (h->tables.flags & GORDER_FLAG_UA_SAMPLES) != 0;
    if (n_edges) {
        if (!p.ua_tiles.empty() && !ua_samples) return refuse("united-atom molecule types");
        if (!p.ua_tiles.empty() && (h->tables.flags & GORDER_FLAG_UA_FAST_NORMALISE))
            return refuse("united-atom molecule types with GORDER_FLAG_UA_FAST_NORMALISE (the fast hydrogen construction is not covered)");
        if (h->extra.maps) return refuse("ordermaps are on");
        if (h->extra.tw) return refuse("timewise is on");
        if (h->dyn) return refuse("dynamic membrane normals");
        if (h->d_ntable) return refuse("a manual normal table is set");
        if (h->manual_frames) return refuse("normals were supplied by gorder_hip_set_normals");
        if (h->n_shells) return refuse("the handle has radial shells");
        if (h->mol.n_groups) return refuse("the handle has molecule rows");
        if (h->nb.on()) return refuse("the handle has neighbour classes");
        if (!p.direct.empty()) return refuse("a bond spans more than the LDS window");
        if (!p.n_acc || (p.tiles.empty() && p.ua_tiles.empty())) return refuse("no bond samples");
        if (const char *why = gorder::hist_edges_check(edges, n_edges)) return refuse(why);
    }
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));       // (a reset still queued may be zeroing the old blocks)
    h->hist.reset();
    h->d_hist_edges.reset();
    h->hist_edges = 0;
    if (!n_edges) return GORDER_OK;
    // replicas against contention on the global words, as the ordinary sums have them (gorder::replica_count)
    const uint32_t n_bins = n_edges - 1u;
    ST_TRY(upload(h, h->d_hist_edges, std::vector<int32_t>(edges, edges + n_edges)));
    ST_TRY(alloc_zeroed(h, h->hist, (size_t)n_bins * 2u * p.n_acc));
    uint32_t max_slots = 1;
    for (const Tile &tile : p.tiles) max_slots = std::max(max_slots, tile.n_slots);
    for (const Tile &tile : p.ua_tiles) max_slots = std::max(max_slots, tile.n_slots);     // (only with GORDER_FLAG_UA_SAMPLES: refused above otherwise)
    const uint32_t planes = h->tables.leaflets.method != GORDER_LEAFLETS_NONE ? 2u : 1u;
    h->hist_table_words = (size_t)planes * n_bins * max_slots;
    h->hist_direct = h->sw.dist_direct || kDistEdgeBytes + h->hist_table_words * sizeof(uint32_t) > 64u * 1024u;
    h->hist_edges = n_edges;
    return GORDER_OK;
}

int gorder_hip_order_histogram_route(gorder_hip_handle *h, uint32_t *direct, uint64_t *table_bytes) {
    if (!h) return GORDER_ERR_INVALID_ARGUMENT;
    if (!h->hist_edges) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_order_histogram_route: the histogram is off");
    if (direct) *direct = h->hist_direct ? 1u : 0u;
    if (table_bytes) *table_bytes = (uint64_t)h->hist_table_words * sizeof(uint32_t);
    return GORDER_OK;
}

int gorder_hip_order_histogram(gorder_hip_handle *h, uint64_t *counts, uint32_t *n_bins) {
    if (!h) return GORDER_ERR_INVALID_ARGUMENT;
    const uint32_t nb = h->hist_edges ? h->hist_edges - 1u : 0u;
    if (n_bins) *n_bins = nb;
    if (!nb) return GORDER_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const uint32_t n = h->plan.n_acc;
    HIP_TRY(h, h->hist.fold(h->stream));
    ST_TRY(gorder_hip_synchronize(h));
    if (!counts) return GORDER_OK;
    std::vector<unsigned long long> raw(h->hist.words);
    HIP_TRY(h, hipMemcpy(raw.data(), h->hist.acc, raw.size() * sizeof(u64), hipMemcpyDeviceToHost));
    const bool lf = h->tables.leaflets.method != GORDER_LEAFLETS_NONE;
    for (uint32_t k = 0; k < nb; k++) {
        const unsigned long long *r = raw.data() + (size_t)k * 2u * n;
        for (uint32_t s = 0; s < n; s++) {
            const uint64_t ctot = r[s], cup = r[n + s];
            const size_t o = (size_t)k * 3u * n + s;
            counts[o] = ctot; counts[o + n] = lf ? cup : 0; counts[o + 2 * (size_t)n] = lf ? ctot - cup : 0;
        }
    }
    return GORDER_OK;
}

// ---- bond reorientation (bond_corr.h, kernels_corr.h) ----------------------------------------------------------------------
int gorder_hip_set_bond_correlation(gorder_hip_handle *h, const uint32_t *lags, uint32_t n_lags) {
    if (!h || (n_lags && !lags)) return GORDER_ERR_INVALID_ARGUMENT;
    const char *who = "gorder_hip_set_bond_correlation: ";
    auto refuse = [&](const std::string &why) { return fail(h, GORDER_ERR_INVALID_ARGUMENT, std::string(who) + why); };
    if (h->collect_locked) return refuse("only before the first submit or prime, or right after gorder_hip_reset");
    const Plan &p = h->plan;
    if (n_lags) {
        if (!p.ua_tiles.empty()) return refuse("united-atom molecule types");
        if (h->extra.geom_kind) return refuse("a geometry selection (a pair may be half inside)");
        if (!p.direct.empty()) return refuse("a bond spans more than the LDS window");
        if (!p.n_acc || p.tiles.empty()) return refuse("no bond samples");
        if (const char *why = gorder::corr_lags_check(lags, n_lags)) return refuse(why);
        const uint64_t plane = gorder::corr_plane_bytes(p.tiles.size(), kBlock);
        if (!gorder::corr_subrange_fit(plane, lags[n_lags - 1], gorder::kCorrRingBudget))
            return refuse("the ring is over budget: (" + std::to_string(lags[n_lags - 1]) + " + 1) planes x " + std::to_string(plane) + " bytes = " +
                          std::to_string(((uint64_t)lags[n_lags - 1] + 1u) * plane) + " bytes > " + std::to_string(gorder::kCorrRingBudget));
    }
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));       // (a reset still queued may be zeroing the old blocks)
    BondCorr &bc = h->corr;
    bc.lags.clear(); bc.d_lags.reset(); bc.ring.reset(); bc.acc.reset();
    bc.ring_planes = bc.subrange = 0; bc.seen = 0;
    if (!n_lags) return GORDER_OK;
    std::vector<uint32_t> padded(lags, lags + n_lags);
    padded.resize((n_lags + gorder::kCorrLagBlock - 1u) / gorder::kCorrLagBlock * gorder::kCorrLagBlock, gorder::kCorrNoLag);
    ST_TRY(upload(h, bc.d_lags, padded));
    ST_TRY(alloc_zeroed(h, bc.acc, (size_t)n_lags * 4u * p.n_acc));
    bc.lags.assign(lags, lags + n_lags);
    return GORDER_OK;
}

int gorder_hip_bond_correlation(gorder_hip_handle *h, int64_t *sums, uint64_t *counts, uint32_t *n_lags) {
    if (!h) return GORDER_ERR_INVALID_ARGUMENT;
    const uint32_t nl = (uint32_t)h->corr.lags.size();
    if (n_lags) *n_lags = nl;
    if (!nl) return GORDER_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, h->corr.acc.fold(h->stream));
    const int st = gorder_hip_synchronize(h);
    if (st != GORDER_OK) return st;
    if (!sums && !counts) return GORDER_OK;
    std::vector<unsigned long long> raw(h->corr.acc.words);
    HIP_TRY(h, hipMemcpy(raw.data(), h->corr.acc.acc, raw.size() * sizeof(u64), hipMemcpyDeviceToHost));
    const bool lf = h->tables.leaflets.method != GORDER_LEAFLETS_NONE;
    const uint32_t n = h->plan.n_acc;
    for (uint32_t k = 0; k < nl; k++) {
        const unsigned long long *r = raw.data() + (size_t)k * 4u * n;
        for (uint32_t s = 0; s < n; s++) {
            const int64_t stot = (int64_t)r[s], sup = (int64_t)r[n + s];
            const uint64_t ctot = r[2u * n + s], cup = r[3u * n + s];
            const size_t o = (size_t)k * 3u * n + s;
            if (sums) { sums[o] = stot; sums[o + n] = lf ? sup : 0; sums[o + 2 * (size_t)n] = lf ? stot - sup : 0; }
            if (counts) { counts[o] = ctot; counts[o + n] = lf ? cup : 0; counts[o + 2 * (size_t)n] = lf ? ctot - cup : 0; }
        }
    }
    return GORDER_OK;
}

// ---- order by local composition (neighbour_classes.h, kernels_neighbours.h) ----------------------------------------------
int gorder_hip_set_neighbour_classes(gorder_hip_handle *h, const uint32_t *centres, const uint32_t *neighbours, uint32_t n_neighbours,
                                     float radius, uint32_t n_classes) {
    if (!h) return GORDER_ERR_INVALID_ARGUMENT;
    const char *who = "gorder_hip_set_neighbour_classes: ";
    auto refuse = [&](const char *why) { return fail(h, GORDER_ERR_INVALID_ARGUMENT, std::string(who) + why); };
    if (h->collect_locked) return refuse("only before the first submit or prime, or right after gorder_hip_reset");
    const Plan &p = h->plan;
    NeighbourClasses &nb = h->nb;
    if (n_neighbours) {
        if (!p.ua_tiles.empty()) return refuse("united-atom molecule types");
        if (!p.direct.empty()) return refuse("direct items: a bond spans more than the LDS window");
        if (!p.n_acc || p.tiles.empty() || !p.n_mol_total) return refuse("no bond samples");
        if (h->extra.maps) return refuse("ordermaps are on");
        if (h->extra.tw) return refuse("timewise is on");
        if (h->n_shells) return refuse("the handle has radial shells");       // (ahead of the selection they come with)
        if (h->extra.geom_kind) return refuse("a geometry selection");
        if (h->dyn) return refuse("dynamic membrane normals");
        if (h->d_ntable) return refuse("a manual normal table is set");
        if (h->manual_frames) return refuse("normals were supplied by gorder_hip_set_normals");
        if (h->mol.n_groups) return refuse("the handle has molecule rows");
        if (h->hist_edges) return refuse("the handle has an order histogram");
        if (const char *why = gorder::neighbour_args_check(centres, p.n_mol_total, neighbours, n_neighbours, radius, n_classes, p.n_atoms))
            return refuse(why);
    }
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));       // (a reset still queued may be zeroing the old blocks)
    nb.n_classes = 0; nb.rows_frames = 0;
    nb.acc.reset(); nb.rows.reset(); nb.d_centres.reset(); nb.d_neighbours.reset();
    nb.centres.clear(); nb.neighbours.clear();
    if (!n_neighbours) return GORDER_OK;
    nb.centres.assign(centres, centres + p.n_mol_total);
    nb.neighbours.assign(neighbours, neighbours + n_neighbours);
    ST_TRY(upload(h, nb.d_centres, nb.centres));
    ST_TRY(upload(h, nb.d_neighbours, nb.neighbours));
    // replicas against contention on the global class words, as the ordinary sums have them (gorder::replica_count)
    ST_TRY(alloc_zeroed(h, nb.acc, (size_t)n_classes * 4u * p.n_acc));
    uint32_t max_slots = 1;
    for (const Tile &tile : p.tiles) max_slots = std::max(max_slots, tile.n_slots);
    const uint32_t planes = h->tables.leaflets.method != GORDER_LEAFLETS_NONE ? 2u : 1u;
    nb.lds_bytes = (size_t)gorder::class_table_bytes(planes, n_classes, max_slots);
    nb.direct = h->sw.nb_direct || !gorder::class_table_fits(planes, n_classes, max_slots);
    nb.radius = radius; nb.thr = local_radius_threshold(radius);
    nb.n_classes = n_classes;
    return GORDER_OK;
}

int gorder_hip_neighbour_classes(gorder_hip_handle *h, int64_t *sums, uint64_t *counts, uint32_t *n_classes) {
    if (!h) return GORDER_ERR_INVALID_ARGUMENT;
    const uint32_t nc = h->nb.n_classes;
    if (n_classes) *n_classes = nc;
    if (!nc) return GORDER_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const uint32_t n = h->plan.n_acc;
    HIP_TRY(h, h->nb.acc.fold(h->stream));
    ST_TRY(gorder_hip_synchronize(h));
    if (!sums && !counts) return GORDER_OK;
    std::vector<unsigned long long> raw(h->nb.acc.words);
    HIP_TRY(h, hipMemcpy(raw.data(), h->nb.acc.acc, raw.size() * sizeof(u64), hipMemcpyDeviceToHost));
    const bool lf = h->tables.leaflets.method != GORDER_LEAFLETS_NONE;
    for (uint32_t k = 0; k < nc; k++) {
        const unsigned long long *r = raw.data() + (size_t)k * 4u * n;
        for (uint32_t s = 0; s < n; s++) {
            const int64_t tot = (int64_t)r[s], up = (int64_t)r[n + s];
            const uint64_t ctot = r[2 * (size_t)n + s], cup = r[3 * (size_t)n + s];
            const size_t o = (size_t)k * 3u * n + s;
            if (sums) { sums[o] = tot; sums[o + n] = lf ? up : 0; sums[o + 2 * (size_t)n] = lf ? tot - up : 0; }
            if (counts) { counts[o] = ctot; counts[o + n] = lf ? cup : 0; counts[o + 2 * (size_t)n] = lf ? ctot - cup : 0; }
        }
    }
    return GORDER_OK;
}

int gorder_hip_neighbour_class_rows(gorder_hip_handle *h, uint8_t *rows, uint32_t *n_frames, uint32_t *n_mol) {
    if (!h) return GORDER_ERR_INVALID_ARGUMENT;
    const uint32_t nf = h->nb.on() ? h->nb.rows_frames : 0u, nm = h->nb.on() ? h->plan.n_mol_total : 0u;
    if (n_frames) *n_frames = nf;
    if (n_mol) *n_mol = nm;
    if (!rows || !nf) return GORDER_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    ST_TRY(gorder_hip_synchronize(h));
    HIP_TRY(h, hipMemcpy(rows, h->nb.rows, (size_t)nf * nm, hipMemcpyDeviceToHost));
    return GORDER_OK;
}

// ---- per-molecule rows (molecule_rows.h, kernels_molrows.h) -------------------------------------------------------------
int gorder_hip_set_molecule_rows(gorder_hip_handle *h, const uint32_t *group_begin, const uint32_t *slots, uint32_t n_groups) {
    if (!h || (n_groups && (!group_begin || !slots))) return GORDER_ERR_INVALID_ARGUMENT;
    const char *who = "gorder_hip_set_molecule_rows: ";
    auto refuse = [&](const char *why) { return fail(h, GORDER_ERR_INVALID_ARGUMENT, std::string(who) + why); };
    if (h->collect_locked) return refuse("only before the first submit or prime, or right after gorder_hip_reset");
    const Plan &p = h->plan;
    gorder::MolRows mol;
    gorder::UaMolRows ua_mol;
    if (n_groups) {
        if (!p.ua_tiles.empty() && !(h->tables.flags & GORDER_FLAG_UA_SAMPLES)) return refuse("united-atom molecule types");
        if (!p.ua_tiles.empty() && (h->tables.flags & GORDER_FLAG_UA_FAST_NORMALISE))
            return refuse("united-atom molecule types with GORDER_FLAG_UA_FAST_NORMALISE (the fast hydrogen construction is not covered)");
        if (h->extra.maps) return refuse("ordermaps are on");
        if (h->extra.tw) return refuse("timewise is on");
        if (h->n_shells) return refuse("the handle has radial shells");
        if (h->hist_edges) return refuse("the handle has an order histogram");
        if (h->nb.on()) return refuse("the handle has neighbour classes");
        if (h->extra.geom_kind) return refuse("a geometry selection");
        if (h->dyn) return refuse("dynamic membrane normals");
        if (h->d_ntable) return refuse("a manual normal table is set");
        if (h->manual_frames) return refuse("normals were supplied by gorder_hip_set_normals");
        if (!p.direct.empty()) return refuse("a bond spans more than the LDS window");
        if (!p.n_acc || (p.tiles.empty() && p.ua_tiles.empty()) || !p.n_mol_total) return refuse("no bond samples");
        std::vector<uint32_t> group_of_slot;
        if (const char *why = gorder::molecule_groups_check(group_begin, slots, n_groups, p.n_acc, group_of_slot)) return refuse(why);
        if ((uint64_t)n_groups * p.n_mol_total > 0xffffffffull) return refuse("groups x molecules exceed 2^32 words a frame");
        gorder::build_molecule_rows(p.tiles, p.items, p.tile_slots, group_of_slot, n_groups, p.n_mol_total, mol);
        if (!p.ua_tiles.empty()) {      // (GORDER_FLAG_UA_SAMPLES) the united-atom tiles' word lists, and their share of the statistics
            std::map<uint32_t, uint32_t> tiles_of_word;
            for (const gorder::MolRun &r : mol.runs) tiles_of_word[r.word]++;       // (a run is one (tile, word) pair)
            gorder::build_ua_molecule_rows(p.ua_tiles, p.ua_items, p.ua_tile_slots, group_of_slot, p.n_mol_total, tiles_of_word, ua_mol);
            mol.n_runs += ua_mol.words.size();
            mol.max_runs_per_tile = std::max(mol.max_runs_per_tile, ua_mol.max_local);
            mol.max_tiles_per_word = 0;
            for (const auto &kv : tiles_of_word) mol.max_tiles_per_word = std::max(mol.max_tiles_per_word, kv.second);
        }
    }
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));       // (copies of a run before the reset may still be writing the chunks)
    h->d_mol_items.reset(); h->d_mol_runs.reset(); h->d_mol_run_begin.reset();
    h->d_ua_mol_lanes.reset(); h->d_ua_mol_words.reset(); h->d_ua_mol_word_begin.reset();
    h->ua_mol = gorder::UaMolRows();
    h->mol = gorder::MolRows();
    h->mol_store.release();
    h->mol_failed = false;
    h->mol_batch_log.clear();
    if (!n_groups) return GORDER_OK;
    int st;
    if ((st = upload(h, h->d_mol_items, mol.items)) != GORDER_OK) return st;
    if ((st = upload(h, h->d_mol_runs, mol.runs)) != GORDER_OK) return st;
    if ((st = upload(h, h->d_mol_run_begin, mol.run_begin)) != GORDER_OK) return st;
    if (ua_mol.on()) {
        if ((st = upload(h, h->d_ua_mol_lanes, ua_mol.lane_words)) != GORDER_OK) return st;
        if ((st = upload(h, h->d_ua_mol_words, ua_mol.words)) != GORDER_OK) return st;
        if ((st = upload(h, h->d_ua_mol_word_begin, ua_mol.word_begin)) != GORDER_OK) return st;
        h->ua_mol = std::move(ua_mol);
    }
    h->mol_store.configure((size_t)n_groups * p.n_mol_total * sizeof(uint64_t), gorder::CollectAlloc{PinnedMem::alloc, PinnedMem::release});
    h->mol = std::move(mol);
    return GORDER_OK;
}

int gorder_hip_molecule_rows_count(gorder_hip_handle *h, uint64_t *n_rows) {
    if (!h || !n_rows) return GORDER_ERR_INVALID_ARGUMENT;
    *n_rows = h->mol.n_groups ? h->mol_store.n_rows() : 0;
    return GORDER_OK;
}

int gorder_hip_molecule_rows_stats(gorder_hip_handle *h, uint64_t *n_runs, uint32_t *max_runs_per_tile, uint32_t *max_tiles_per_word) {
    if (!h) return GORDER_ERR_INVALID_ARGUMENT;
    if (!h->mol.n_groups) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_molecule_rows_stats: molecule rows are off");
    if (n_runs) *n_runs = h->mol.n_runs;
    if (max_runs_per_tile) *max_runs_per_tile = h->mol.max_runs_per_tile;
    if (max_tiles_per_word) *max_tiles_per_word = h->mol.max_tiles_per_word;
    return GORDER_OK;
}

int gorder_hip_molecule_rows(gorder_hip_handle *h, int32_t *sums, uint32_t *counts, uint64_t *frames, uint64_t capacity_rows) {
    if (!h) return GORDER_ERR_INVALID_ARGUMENT;
    if (!h->mol.n_groups) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_molecule_rows: molecule rows are off");
    const int st = gorder_hip_synchronize(h);           // (a device error of the run also drops the failed batch's rows)
    if (st != GORDER_OK) return st;
    const gorder::CollectStore &store = h->mol_store;
    if ((sums || counts || frames) && capacity_rows < store.n_rows())
        return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_molecule_rows: capacity_rows is too small");
    if (frames) std::copy(store.frames().begin(), store.frames().end(), frames);
    const size_t wpf = (size_t)h->mol.n_groups * h->plan.n_mol_total;
    if (sums || counts)
        store.for_each_row([&](uint64_t r, const void *row) {
            const uint64_t *w = static_cast<const uint64_t *>(row);
            for (size_t q = 0; q < wpf; q++) {
                int64_t s;
                uint64_t c;
                gorder::molecule_word_unpack(w[q], s, c);
                if (sums) sums[r * wpf + q] = (int32_t)s;
                if (counts) counts[r * wpf + q] = (uint32_t)c;
            }
        });
    return GORDER_OK;
}

int gorder_hip_collected_counts(gorder_hip_handle *h, uint64_t *n_leaflet_rows, uint64_t *n_normal_rows) {
    if (!h) return GORDER_ERR_INVALID_ARGUMENT;
    if (n_leaflet_rows) *n_leaflet_rows = (h->collect & GORDER_COLLECT_LEAFLETS) ? h->collect_flags.n_rows() : 0;
    if (n_normal_rows) *n_normal_rows = (h->collect & GORDER_COLLECT_NORMALS) ? h->collect_normals.n_rows() : 0;
    return GORDER_OK;
}

int gorder_hip_collected_leaflets(gorder_hip_handle *h, uint8_t *flags, uint64_t *frames, uint64_t capacity_rows, uint64_t *n_rows) {
    if (!h || !n_rows) return GORDER_ERR_INVALID_ARGUMENT;
    *n_rows = 0;
    if (!(h->collect & GORDER_COLLECT_LEAFLETS)) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_collected_leaflets: leaflets are not being collected");
    const gorder::CollectStore &store = h->collect_flags;
    *n_rows = store.n_rows();
    if ((flags || frames) && capacity_rows < store.n_rows()) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_collected_leaflets: capacity_rows is too small");
    const int st = gorder_hip_synchronize(h);       // the copies into the chunks are behind the batches' kernels on the stream
    if (st != GORDER_OK) return st;
    const size_t n_mol = h->plan.n_mol_total;
    if (flags)
        store.for_each_row([&](uint64_t r, const void *row) {
            gorder::collect_unpack_flags(static_cast<const uint64_t *>(row), n_mol, flags + r * n_mol);
        });
    if (frames && store.n_rows()) memcpy(frames, store.frames().data(), store.n_rows() * sizeof(uint64_t));
    return GORDER_OK;
}

int gorder_hip_collected_normals(gorder_hip_handle *h, float *normals, uint64_t *frames, uint64_t capacity_rows, uint64_t *n_rows) {
    if (!h || !n_rows) return GORDER_ERR_INVALID_ARGUMENT;
    *n_rows = 0;
    if (!(h->collect & GORDER_COLLECT_NORMALS)) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_collected_normals: normals are not being collected");
    const gorder::CollectStore &store = h->collect_normals;
    *n_rows = store.n_rows();
    if ((normals || frames) && capacity_rows < store.n_rows()) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_collected_normals: capacity_rows is too small");
    ST_TRY(gorder_hip_synchronize(h));
    const size_t row_floats = (size_t)h->plan.n_mol_total * 3u;
    if (normals)
        store.for_each_row([&](uint64_t r, const void *row) { memcpy(normals + r * row_floats, row, row_floats * sizeof(float)); });
    if (frames && store.n_rows()) memcpy(frames, store.frames().data(), store.n_rows() * sizeof(uint64_t));
    return GORDER_OK;
}

int gorder_hip_leaflet_distances(gorder_hip_handle *h, float *dist) {
    if (!h || !dist || !h->d_adist) return GORDER_ERR_INVALID_ARGUMENT;
    ST_TRY(gorder_hip_synchronize(h));
    HIP_TRY(h, hipMemcpy(dist, h->d_adist, sizeof(float) * h->plan.n_mol_total, hipMemcpyDeviceToHost));
    return GORDER_OK;
}

int gorder_hip_spherical_stats(gorder_hip_handle *h, float out[12]) {
    if (!h || !out || h->tables.leaflets.method != GORDER_LEAFLETS_SPHERICAL || !h->d_sph_stats) return GORDER_ERR_INVALID_ARGUMENT;
    if (!h->have_assignment) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_spherical_stats: no assignment frame yet");
    ST_TRY(gorder_hip_synchronize(h));
    HIP_TRY(h, hipMemcpy(out, h->d_sph_stats, 12 * sizeof(float), hipMemcpyDeviceToHost));
    return GORDER_OK;
}

int gorder_hip_clustering_stats(gorder_hip_handle *h, float out[12]) {
    if (!h || !out || h->tables.leaflets.method != GORDER_LEAFLETS_CLUSTERING || !h->d_cl_stats) return GORDER_ERR_INVALID_ARGUMENT;
    if (!h->have_assignment) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_clustering_stats: no assignment frame yet");
    ST_TRY(gorder_hip_synchronize(h));
    HIP_TRY(h, hipMemcpy(out, h->d_cl_stats, 12 * sizeof(float), hipMemcpyDeviceToHost));
    return GORDER_OK;
}

int gorder_hip_accumulators_device(gorder_hip_handle *h, void **d_ptr, uint64_t *n_u64) {
    if (!h || !d_ptr || !n_u64) return GORDER_ERR_INVALID_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    ST_TRY(fold_replicas(h));      // the packed block must be complete before a collective reads it (stream-ordered)
    *d_ptr = h->d_acc;
    *n_u64 = h->acc_words;
    return GORDER_OK;
}

int gorder_hip_export_maps(gorder_hip_handle *h, void *d_sums, void *d_counts, uint64_t n_u64) {
    if (!h || !h->extra.maps || !d_sums || !d_counts) return GORDER_ERR_INVALID_ARGUMENT;
    const uint64_t n = 3ull * h->plan.n_acc * h->map_nx * h->map_ny;
    if (n_u64 < n) return GORDER_ERR_INVALID_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    ST_TRY(fold_maps(h));
    HIP_TRY(h, hipMemcpyAsync(d_sums, h->d_map_sums, n * sizeof(unsigned long long), hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(d_counts, h->d_map_cnts, n * sizeof(unsigned long long), hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return check_device_error(h);
}

int gorder_hip_bind_accumulators(gorder_hip_handle *h, void *d_ptr, uint64_t n_u64) {
    if (!h || !d_ptr || n_u64 < h->acc_words || ((uintptr_t)d_ptr & 7u)) return GORDER_ERR_INVALID_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    ST_TRY(fold_replicas(h));
    HIP_TRY(h, hipMemcpyAsync(d_ptr, h->d_acc, h->acc_words * sizeof(unsigned long long), hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->own_acc.reset();
    h->d_acc = (unsigned long long *)d_ptr;
    return GORDER_OK;
}

// ---- a fresh SystemTopology on the same tables --------------------------------------------------------------------
int gorder_hip_reset(gorder_hip_handle *h) {
    if (!h) return GORDER_ERR_INVALID_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    const Plan &p = h->plan;
    HIP_TRY(h, hipMemsetAsync(h->d_acc, 0, h->acc_words * sizeof(unsigned long long), h->stream));
    if (h->d_rep) HIP_TRY(h, hipMemsetAsync(h->d_rep, 0, (size_t)h->sw.replicas * 4u * p.n_acc * sizeof(unsigned long long), h->stream));
    h->rep_dirty = false;
    if (h->n_shells) HIP_TRY(h, h->shells.zero_async(h->stream));       // (the radii stay)
    if (h->hist_edges) HIP_TRY(h, h->hist.zero_async(h->stream));      // (the edges stay)
    if (h->nb.on()) {       // (the setting stays; the class rows are those of a batch of the run that ends here)
        HIP_TRY(h, h->nb.acc.zero_async(h->stream));
        h->nb.rows_frames = 0;
    }
    if (h->corr.on()) {     // (the lags and the ring stay; its planes are history no pair will ask for)
        HIP_TRY(h, h->corr.acc.zero_async(h->stream));
        h->corr.seen = 0;
    }
    if (h->extra.maps) {
        const size_t nmap = 3 * (size_t)p.n_acc * h->map_nx * h->map_ny;
        const size_t npk = (h->tables.leaflets.method != GORDER_LEAFLETS_NONE ? 2 : 1) * (nmap / 3);
        HIP_TRY(h, hipMemsetAsync(h->d_map_sums, 0, nmap * sizeof(unsigned long long), h->stream));
        HIP_TRY(h, hipMemsetAsync(h->d_map_cnts, 0, nmap * sizeof(unsigned long long), h->stream));
        HIP_TRY(h, hipMemsetAsync(h->d_map_packed, 0, npk * sizeof(unsigned long long), h->stream));
        h->map_pending = 0;
    }
    if (h->d_tw_sums) {
        const size_t n = h->tw_cap * 3 * (size_t)p.n_acc * sizeof(unsigned long long);
        HIP_TRY(h, hipMemsetAsync(h->d_tw_sums, 0, n, h->stream));
        HIP_TRY(h, hipMemsetAsync(h->d_tw_cnts, 0, n, h->stream));
    }
    HIP_TRY(h, hipMemsetAsync(h->d_err, 0xff, kErrWords * sizeof(uint32_t), h->stream));
    h->batch_log.clear();
    h->n_frames = 0;
    // collected rows: gone (the chunks stay, copies still queued into them run before anything a later batch queues); the
    // switch stays and may be set anew
    h->collect_flags.clear();
    h->collect_normals.clear();
    h->mol_store.clear();                  // (the groups stay)
    h->mol_failed = false;
    h->mol_batch_log.clear();
    h->collect_locked = false;
    h->have_assignment = false;
    h->cl_have_carry = false;
    h->replay_have_carry = false;          // (the tables stay)
    h->assignment_frame = 0;
    h->manual_frames = 0;
    h->err_index = 0;
    h->err_msg.clear();
    // a new run speculates again (and starts its statistics anew); the batches still in flight are waited for first —
    // their counters would otherwise be booked on the new run
    if (h->d_own) {
        spec_poll(h, true);
        h->spec_enabled = true;
        h->spec_batches = h->spec_fixed = h->spec_exact_frames = 0;
        HIP_TRY(h, hipMemsetAsync(h->d_spec_counters, 0, 4 * sizeof(uint32_t), h->stream));
    }
    // likewise k_local_decide: a new run tries the bound again (a report still in flight is read, and dropped)
    if (h->d_lsummary) {
        if (h->lsummary_pending) { (void)hipEventSynchronize(h->lsummary_written); h->lsummary_pending = false; }
        h->decide_pause = 0;
        h->decide_submits = h->decide_paused_submits = 0;
        h->h_lsummary[0] = h->h_lsummary[1] = 0u;
        HIP_TRY(h, hipMemsetAsync(h->d_lsummary, 0, 2 * sizeof(uint32_t), h->stream));
    }
    return GORDER_OK;
}

int gorder_hip_comm_unique_id(uint8_t id[128]) {
    if (!id) return GORDER_ERR_INVALID_ARGUMENT;
    RcclApi *api = rccl_api(nullptr);
    if (!api) return GORDER_ERR_DEVICE;
    UniqueId u;
    if (api->get_unique_id(&u) != 0) return GORDER_ERR_DEVICE;
    memcpy(id, u.internal, 128);
    return GORDER_OK;
}

int gorder_hip_comm_create(gorder_hip_handle *h, const uint8_t id[128], int n_ranks, int rank, void **comm_out) {
    if (!h || !id || !comm_out || n_ranks < 1 || rank < 0 || rank >= n_ranks) return GORDER_ERR_INVALID_ARGUMENT;
    *comm_out = nullptr;
    std::string why;
    RcclApi *api = rccl_api(&why);
    if (!api) return fail(h, GORDER_ERR_DEVICE, why);
    HIP_TRY(h, hipSetDevice(h->device));
    UniqueId u;
    memcpy(u.internal, id, 128);
    const int rc = api->comm_init_rank(comm_out, n_ranks, u, rank);
    if (rc != 0) return fail(h, GORDER_ERR_DEVICE, rccl_error(api, "ncclCommInitRank", rc));
    return GORDER_OK;
}

void gorder_hip_comm_destroy(void *comm) {
    RcclApi *api = rccl_api(nullptr);
    if (api && comm) (void)api->comm_destroy(comm);
}

int gorder_hip_allreduce(gorder_hip_handle *h, void *nccl_comm) {
    if (!h || !nccl_comm) return GORDER_ERR_INVALID_ARGUMENT;
    std::string why;
    RcclApi *api = rccl_api(&why);
    if (!api) return fail(h, GORDER_ERR_DEVICE, why);
    HIP_TRY(h, hipSetDevice(h->device));
    int st = fold_replicas(h);
    if (st != GORDER_OK) return st;
    if ((st = fold_maps(h)) != GORDER_OK) return st;
    // everything that SystemTopology::add sums (topology/mod.rs:236-254) in one group on the handle's stream: the packed
    // accumulator block (order sums, counts, total_frames) and, with ordermaps, the folded i64 / u64 maps (Map::add,
    // ordermap.rs:116-138).  Integer sums: the result is bit-identical whatever the ring order.
    int rc = api->group_start();
    if (rc == 0) rc = api->all_reduce(h->d_acc, h->d_acc, h->acc_words, kNcclInt64, kNcclSum, nccl_comm, h->stream);
    if (rc == 0 && h->extra.maps) {
        const size_t nmap = 3 * (size_t)h->plan.n_acc * h->map_nx * h->map_ny;
        rc = api->all_reduce(h->d_map_sums, h->d_map_sums, nmap, kNcclInt64, kNcclSum, nccl_comm, h->stream);
        if (rc == 0) rc = api->all_reduce(h->d_map_cnts, h->d_map_cnts, nmap, kNcclInt64, kNcclSum, nccl_comm, h->stream);
    }
    const int rc_end = api->group_end();
    if (rc == 0) rc = rc_end;
    if (rc != 0) return fail(h, GORDER_ERR_DEVICE, rccl_error(api, "ncclAllReduce", rc));
    return GORDER_OK;
}

uint64_t gorder_hip_last_error_index(const gorder_hip_handle *h) { return h ? h->err_index : 0; }
uint64_t gorder_hip_last_error_frame(const gorder_hip_handle *h) { return h ? h->err_frame : 0; }
const char *gorder_hip_kernel_time_names(const gorder_hip_handle *h) { return h ? h->timed_kernels.c_str() : ""; }
const char *gorder_hip_last_error_message(const gorder_hip_handle *h) { return h ? h->err_msg.c_str() : ""; }

int gorder_hip_kernel_time(gorder_hip_handle *h, double *ms, uint64_t *launches, int reset) {
    if (!h) return GORDER_ERR_INVALID_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    h->timing_on = true;   // the first call switches the events on (submits before it are not timed)
    while (!h->timing_pending.empty()) {
        ST_TRY(timing_drain_oldest(h));
    }
    double total = 0.0;
    for (double v : h->timing_label_ms) total += v;
    if (ms) *ms = total;
    if (launches) *launches = h->timing_launches;
    if (reset) {
        h->timing_labels.clear(); h->timing_label_ms.clear(); h->timing_label_n.clear();
        h->timed_kernels.clear();
        h->timing_launches = 0;
        h->timing_open_label = -1;       // (a segment left open — there is none between submits — would name a label that is gone)
    }
    return GORDER_OK;
}

int gorder_hip_kernel_time_group(gorder_hip_handle *h, uint32_t index, const char **name, double *ms, uint64_t *segments) {
    if (!h) return GORDER_ERR_INVALID_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    while (!h->timing_pending.empty()) {
        ST_TRY(timing_drain_oldest(h));
    }
    if (index >= h->timing_labels.size()) return GORDER_ERR_INVALID_ARGUMENT;
    if (name) *name = h->timing_labels[index].c_str();
    if (ms) *ms = h->timing_label_ms[index];
    if (segments) *segments = h->timing_label_n[index];
    return GORDER_OK;
}

// ---- XTC frames decompressed on the device (kernels_xtc.h) ---------------------------------------------------------
// checkpoints a batch needs between its two kernels
size_t xtc_checkpoints(uint32_t n_frames, uint32_t n_stop) {
    return (size_t)n_frames * ((std::max(n_stop, 1u) + kXtcChunk - 1u) / kXtcChunk + 1u);
}
// `kinds`: what the table holds — kXtcTableXtc: frames for k_xtc_scan / k_xtc_chunks, kXtcTableTrr: frames for k_trr_unpack
// (each kernel passes over the frames of the other kind); a kind the table does not hold queues nothing
enum : uint32_t { kXtcTableXtc = 1u, kXtcTableTrr = 2u };
uint32_t xtc_table_kinds(const gorder_xtc_frame_t *frames, uint32_t n_frames) {
    uint32_t kinds = 0;
    for (uint32_t k = 0; k < n_frames; k++) kinds |= (frames[k].kind & (kTrrKindF32 | kTrrKindF64)) ? kXtcTableTrr : kXtcTableXtc;
    return kinds;
}
int xtc_decode_on(gorder_hip_handle *h, hipStream_t stream, const uint8_t *d_blob, uint64_t blob_bytes,
                  const gorder_xtc_frame_t *d_frames, uint32_t n_frames, uint32_t n_atoms_file, const int32_t *d_slot_of,
                  uint32_t n_stop, float *d_xyz, uint32_t n_atoms_out, uint32_t kinds, uint32_t *d_stat = nullptr,
                  uint32_t *d_short = nullptr, uint32_t *d_err_key = nullptr, XtcCheckpoint *d_cp = nullptr) {
    if (!h || !d_blob || !d_frames || !d_xyz || blob_bytes < 64 || (reinterpret_cast<uintptr_t>(d_blob) & 63u) != 0 || n_atoms_file == 0 || n_atoms_out == 0 ||
        n_stop > n_atoms_file || (!d_slot_of && n_atoms_out < n_stop))
        return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_xtc_decode: bad arguments");
    if (n_frames == 0) return GORDER_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    if (kinds & kXtcTableXtc) {
        // two kernels (kernels_xtc.h): where the chunks of ~kXtcChunk atoms start in every frame's stream (one lane per
        // frame, no decoding), then the chunks (one lane per frame and chunk).  The checkpoints between them live in the
        // caller's buffer (a slot of gorder_hip_run_trajectory has its own: several batches decode at once) or the handle's.
        const uint32_t n_chunks = (std::max(n_stop, 1u) + kXtcChunk - 1u) / kXtcChunk;
        if (!d_cp) {
            ST_TRY(ensure(h, h->d_xtc_cp, xtc_checkpoints(n_frames, n_stop)));
            d_cp = h->d_xtc_cp;
        }
        hipLaunchKernelGGL(k_xtc_scan, dim3((n_frames + 3u) / 4u), dim3(256), 0, stream, d_blob, (unsigned long long)blob_bytes,
                           d_frames, n_frames, n_atoms_file, d_slot_of, n_stop, d_xyz, n_atoms_out,
                           d_err_key ? d_err_key : h->d_err, d_stat, d_short, d_cp, n_chunks);
        const unsigned long long items = (unsigned long long)n_frames * n_chunks;
        if (items + 63ull > 64ull * 0x7fffffffull) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_xtc_decode: batch too large");
        hipLaunchKernelGGL(k_xtc_chunks, dim3((uint32_t)((items + 63ull) / 64ull)), dim3(64), 0, stream, d_blob,
                           (unsigned long long)blob_bytes, d_frames, n_frames, n_atoms_file, d_slot_of, n_stop, d_xyz, n_atoms_out,
                           d_cp, n_chunks);
    }
    if (kinds & kXtcTableTrr) {
        // one kernel (kernels_trr.h): a thread per four floats of a frame's stream (per atom with a slot table), the frames
        // along the grid's second axis; timed as a group of its own where it runs on the handle's stream
        const unsigned long long items = d_slot_of ? std::max(n_stop, 1u) : (3ull * n_stop) / 4ull + 1ull;
        const uint32_t pieces = (uint32_t)std::min<unsigned long long>((items + kTrrBlock - 1u) / kTrrBlock, 0x7fffffffull);
        const bool timed = stream == h->stream;
        if (timed) TIMING_MARK(h, "k_trr_unpack");
        hipLaunchKernelGGL(k_trr_unpack, dim3(pieces, std::min(n_frames, 65535u)), dim3(kTrrBlock), 0, stream, d_blob,
                           (unsigned long long)blob_bytes, d_frames, n_frames, n_atoms_file, d_slot_of, n_stop, d_xyz, n_atoms_out,
                           d_err_key ? d_err_key : h->d_err);
        if (timed) TIMING_MARK(h, nullptr);
    }
    HIP_TRY(h, hipGetLastError());
    return GORDER_OK;
}
int gorder_hip_xtc_decode(gorder_hip_handle *h, const uint8_t *d_blob, uint64_t blob_bytes,
                          const gorder_xtc_frame_t *d_frames, uint32_t n_frames, uint32_t n_atoms_file,
                          const int32_t *d_slot_of, uint32_t n_stop, float *d_xyz, uint32_t n_atoms_out) {
    if (!h) return GORDER_ERR_INVALID_ARGUMENT;
    if (!d_frames) return fail(h, GORDER_ERR_INVALID_ARGUMENT, "gorder_hip_xtc_decode: bad arguments");
    // which kernels the table needs: its `kind` words, read back in the order of the handle's stream (the table is the
    // caller's, on the device) — the call waits for what the stream holds so far, the kernels themselves are asynchronous
    HIP_TRY(h, hipSetDevice(h->device));
    std::vector<uint32_t> kind(n_frames);
    if (n_frames) {
        HIP_TRY(h, hipMemcpy2DAsync(kind.data(), sizeof(uint32_t), reinterpret_cast<const uint8_t *>(d_frames) + offsetof(gorder_xtc_frame_t, kind),
                                    sizeof(gorder_xtc_frame_t), sizeof(uint32_t), n_frames, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    uint32_t kinds = 0;
    for (uint32_t k : kind) kinds |= (k & (kTrrKindF32 | kTrrKindF64)) ? kXtcTableTrr : kXtcTableXtc;
    return xtc_decode_on(h, h->stream, d_blob, blob_bytes, d_frames, n_frames, n_atoms_file, d_slot_of, n_stop, d_xyz,
                         n_atoms_out, kinds);
}

}  // extern "C"

#include "trajectory_driver.h"
