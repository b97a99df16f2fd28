/*
 * gorder_hip.h — C ABI of the MI355X (gfx950) lipid-order engine.
 *
 * This is the drop-in boundary for ONE path of VachaLab/gorder: the per-frame
 * order-parameter computation that gorder runs inside
 *   groan_rs `System::traj_iter_map_reduce(.., body = analyze_frame, ..)`
 *   (call sites  src/analysis/common.rs:283-339, body  src/analysis/common.rs:201-235,
 *    data type  `SystemTopology`  src/analysis/topology/mod.rs:34-65,
 *    map/reduce trait impl  src/analysis/topology/mod.rs:256-278).
 *
 * Mapping of the reference's interface onto this ABI
 *   SystemTopology::new  (topology/mod.rs:70-118)        -> gorder_hip_create
 *   ParallelTrajData::initialize (topology/mod.rs:274-277) -> one handle per GPU/rank; the caller
 *                                                            passes GLOBAL frame indices to submit
 *   analyze_frame (common.rs:201-235), called per frame   -> gorder_hip_submit_{device,host}, called
 *                                                            per BATCH of frames (AoS xyz as decoded)
 *   SystemTopology::add / reduce (topology/mod.rs:236-272) -> gorder_hip_finish returns raw i64 sums +
 *                                                            u64 counts which add element-wise
 *                                                            (order.rs:160-176, ordermap.rs:116-138);
 *                                                            on a multi-GPU node one RCCL all-reduce
 *                                                            (gorder_hip_allreduce, or the host's own
 *                                                            over gorder_hip_accumulators_device())
 *   read_trajectory (common.rs:239-342)                    -> gorder_hip_run_trajectory
 *   Result<(), AnalysisError> (errors.rs:121-168)          -> gorder_status_t + gorder_hip_last_error_index
 *
 * Plain pointers and sizes only.  No allocation ownership crosses the boundary: every input
 * buffer stays owned by the caller, every output buffer is caller-allocated.
 * A handle is thread-compatible (one handle per host thread / GPU / stream), exactly like one
 * `SystemTopology` clone per thread in the reference.
 */
#ifndef GORDER_HIP_H
#define GORDER_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "gorder_xtc.h"   /* gorder_xtc_frame_t for gorder_hip_xtc_decode */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---------------------------------------------------------------------------
 * 1..9 mirror the AnalysisError variants the per-frame path can raise (src/errors.rs:121-141).
 * >= 100 are errors of this library (no counterpart in the reference). */
typedef enum {
    GORDER_OK = 0,
    GORDER_ERR_UNDEFINED_BOX = 1,                   /* AnalysisError::UndefinedBox            errors.rs:124 */
    GORDER_ERR_NOT_ORTHOGONAL_BOX = 2,              /* AnalysisError::NotOrthogonalBox        errors.rs:128 */
    GORDER_ERR_ZERO_BOX = 3,                        /* AnalysisError::ZeroBox                 errors.rs:132 */
    GORDER_ERR_UNDEFINED_POSITION = 4,              /* AnalysisError::UndefinedPosition(idx)  errors.rs:136 */
    GORDER_ERR_INVALID_GLOBAL_MEMBRANE_CENTER = 5,  /* ...::InvalidGlobalMembraneCenter       errors.rs:139 */
    GORDER_ERR_INVALID_LOCAL_MEMBRANE_CENTER = 6,   /* ...::InvalidLocalMembraneCenter(idx)   errors.rs:143 */
    GORDER_ERR_DYNAMIC_NORMAL = 7,                  /* ...::DynamicNormalError(NotEnoughPoints(n)) errors.rs:155,
                                                       172-177; gorder_hip_last_error_index = n */
    GORDER_ERR_MANUAL_LEAFLET_FRAME = 8,            /* ManualLeafletClassificationError::FrameNotFound: a frame of the batch has
                                                       no row in the manual leaflet table; gorder_hip_last_error_frame */
    GORDER_ERR_MANUAL_NORMAL_FRAME = 9,             /* ManualNormalError::FrameNotFound: the same for the manual normal table */
    GORDER_ERR_INVALID_ARGUMENT = 100,
    GORDER_ERR_DEVICE = 101,          /* a HIP runtime call failed; see gorder_hip_last_error_message */
    GORDER_ERR_NO_DEVICE = 102,       /* no gfx950 device visible: the product path has NO CPU fallback */
    GORDER_ERR_BOX_RANGE = 103,       /* a box edge is <= 0 / NaN, or a coordinate lies so far outside
                                         the box that the reference's `while` minimum-image loop would not
                                         terminate in 8 iterations (the reference would spin) */
    GORDER_ERR_LEAFLETS_NOT_PRIMED = 104, /* first submitted frame is not an assignment frame and no
                                             earlier assignment is known: call gorder_hip_prime_leaflets */
    GORDER_ERR_OVERFLOW = 105,        /* a batch was refused because frames x molecules would reach 2^63 / 1e6: an i64
                                         order sum could then overflow (the reference panics, order.rs:44-60) */
    GORDER_ERR_TRAJECTORY_FORMAT = 106,/* a corrupt or truncated trajectory frame, met by gorder_hip_xtc_decode on the device or
                                         by the host reader inside gorder_hip_run_trajectory (the reference: a read error
                                         of the trajectory iterator, common.rs:248) */
    GORDER_ERR_CLUSTERING = 107,      /* GORDER_LEAFLETS_SPHERICAL: a head-centre distance of an assignment frame is not finite
                                         (the reference panics in the sort of spherical_clustering.rs:120);
                                         GORDER_LEAFLETS_CLUSTERING: a coordinate of a group atom or a distance between two
                                         of them is not finite; gorder_hip_last_error_index = that frame */
    GORDER_ERR_CLUSTER_MATCH = 108    /* GORDER_LEAFLETS_CLUSTERING: the clusters of an assignment frame overlap neither leaflet
                                         of the previous assignment frame by 80 % (ClusterError::CouldNotMatchLeaflets(80),
                                         clustering.rs:770-785); gorder_hip_last_error_index = that frame */
} gorder_status_t;

/* ---- leaflets -------------------------------------------------------------------------------- */
typedef enum {
    GORDER_LEAFLETS_NONE = 0,
    GORDER_LEAFLETS_GLOBAL = 1,      /* leaflets.rs:171-205 + :711-732 */
    GORDER_LEAFLETS_LOCAL = 2,       /* leaflets.rs:661-675 + pbc.rs:273-318 + :711-732 */
    GORDER_LEAFLETS_INDIVIDUAL = 3,  /* leaflets.rs:777-801 */
    GORDER_LEAFLETS_MANUAL = 4,      /* host supplies flags per assignment frame (leaflets.rs:820-860);
                                        Leaflet encoding Upper=0, Lower=1 (lib.rs:416-422) */
    GORDER_LEAFLETS_SPHERICAL = 5,   /* LeafletClassification::spherical_clustering (spherical_clustering.rs:42-277, leaflets.rs:
                                        1296-1366), for vesicles: per assignment frame the centre of geometry of the group
                                        "ClusterHeads", every group atom's distance to it, a two-component 1-D Gaussian mixture
                                        fitted to the distances by EM; the component farther out is the upper leaflet.
                                        `membrane` / `n_membrane` carry the group (every atom the heads query selects, ascending —
                                        the order matters only for reproducibility; at least 2, leaflets.rs:106-115), each
                                        molecule's `heads[k]` is its own atom of that group; normal_dim and radius are unused,
                                        frequency and flip as for the other methods */
    GORDER_LEAFLETS_CLUSTERING = 6   /* LeafletClassification::clustering (clustering.rs:478-800), spectral clustering for membranes
                                        of any shape (buckled, tubes, wrapped around the box).  Per assignment frame, over the n
                                        atoms of "ClusterHeads" in ascending order: W_ij = expf(-d_ij^2) (sigma = 1, 3-D minimum
                                        image with handle_pbc, no cut-off), deg = W 1, L = I - D^-1/2 W D^-1/2; the eigenvectors
                                        of L's 2nd and 3rd smallest eigenvalues, rows normalised; 2-means from rows 0 and 1
                                        (100 rounds at most, ties to cluster 0); frame 0: the more populated cluster is upper
                                        (tie: the one with the lowest atom), later frames: the cluster is what 80 % of it was in
                                        the previous assignment frame, else GORDER_ERR_CLUSTER_MATCH.
                                        "Skip the first" is exact here: L's eigenvector of eigenvalue 0 is D^1/2 1 in closed
                                        form, the device deflates that vector and takes the next two (the reference takes
                                        columns 1 and 2 of a full decomposition, an arbitrary basis where the cross-leaflet
                                        weights underflow and eigenvalue 0 is double).  ONE definition runs for every frame:
                                        the reference's sloppy route (cut-off, sigma 0.5, random Lanczos start, retries), its
                                        switching rules and its thread-shared reference clusters are CPU cost heuristics whose
                                        result is "the precise result, when they succeed", and are not reproduced.
                                        `membrane` / `n_membrane` carry the group, ascending and distinct, 2 <= n_membrane <=
                                        8192 (dense route: the scratch holds n x 301 floats a frame, 512 MiB at most);
                                        with GORDER_FLAG_CLUSTER_CUTOFF (below) 2 <= n_membrane <= 131072: the same definition
                                        with W_ij = 0 where d_ij^2 >= 36 nm^2, spread over the device;
                                        each molecule's heads[k] is its own atom of the group; normal_dim and radius unused */
} gorder_leaflet_method_t;

typedef struct {
    uint32_t method;        /* gorder_leaflet_method_t */
    uint32_t normal_dim;    /* 0=x 1=y 2=z : `membrane_normal: Dimension` of the classifier */
    uint32_t frequency;     /* 0 = Frequency::Once, n>=1 = Frequency::Every(n); this is the REAL
                               frequency = input frequency * step (leaflets.rs:157-163) */
    uint32_t flip;          /* leaflets.rs:68-73 */
    float radius;           /* Local: cylinder radius in nm (leaflets.rs:389-418) */
    uint32_t n_membrane;    /* Global/Local: size of group "Membrane"; Spherical: size of group "ClusterHeads" (>= 2) */
    const uint32_t *membrane; /* atom indices (into the submitted coordinate frame); Spherical: the atoms of "ClusterHeads",
                                 among them every molecule's heads[k] */
} gorder_leaflets_t;

/* ---- ordermaps (src/analysis/ordermap.rs:40-113, input/ordermap.rs:34-50) --------------------- */
typedef struct {
    uint32_t enabled;
    uint32_t plane;         /* 0=xy, 1=xz, 2=yz (yz projects to (z, y), input/ordermap.rs:48) */
    float span_x[2];        /* resolved span; GridSpan::Auto => (0, box) of the STRUCTURE file */
    float span_y[2];
    float bin[2];
} gorder_ordermap_t;

/* ---- molecule types ---------------------------------------------------------------------------
 * United-atom carbon kinds (uaorder.rs:448-452). */
typedef enum {
    GORDER_UA_CH1_SAT = 1,   /* indices = helper1, helper2, helper3, target  (uaorder.rs:1050-1055) */
    GORDER_UA_CH2 = 2,       /* indices = helper1, target, helper2, -        (uaorder.rs:911-915)  */
    GORDER_UA_CH3 = 3,
    GORDER_UA_CH1_UNSAT = 4
} gorder_ua_kind_t;

typedef struct {
    uint32_t kind;             /* gorder_ua_kind_t; number of virtual C-H bonds = 1,2,3,1 */
    const uint32_t *indices;   /* [n_molecules][4] */
} gorder_ua_atom_t;

typedef struct {
    uint32_t n_molecules;
    /* AA / CG (BondType, topology/bond.rs:220-246): */
    uint32_t n_bond_types;
    const uint32_t *bonds;     /* [n_bond_types][n_molecules][2] atom indices, first < second
                                  (bond.rs:300-304, 338-344) */
    /* UA (UAOrderAtoms, topology/uatom.rs): */
    uint32_t n_ua_atoms;
    const gorder_ua_atom_t *ua_atoms;
    /* leaflet classifier inputs (leaflets.rs:575-590, 744-775): */
    const uint32_t *heads;     /* [n_molecules] or NULL */
    uint32_t n_methyls;        /* equal for all molecules of a type (leaflets.rs:760-770) */
    const uint32_t *methyls;   /* [n_molecules][n_methyls] or NULL */
    /* dynamic membrane normal (normal.rs:145-158, get_reference_head): */
    const uint32_t *normal_heads; /* [n_molecules] the molecule's atom of group "NormalHeads", or NULL */
} gorder_moltype_t;

/* ---- dynamic membrane normals (src/analysis/normal.rs:160-199, 421-458; pbc.rs:142-161, 321-350) ----
 * Per frame and molecule: the cloud of "NormalHeads" atoms within `radius` (3-D, minimum image) of the
 * molecule's own head, made whole around it; the normal is the direction of least variance of the cloud
 * (last right singular vector of the demeaned cloud).  Fewer than 3 points: GORDER_ERR_DYNAMIC_NORMAL,
 * raised only if a sample of that molecule is actually accumulated (the reference computes normals lazily,
 * after the geometry test, bond.rs:424-431).  With `enabled` the static `normal` of the tables is unused. */
typedef struct {
    uint32_t enabled;
    float radius;
    uint32_t n_cloud;
    const uint32_t *cloud;     /* atom indices of group "NormalHeads" (every atom the heads query selects) */
} gorder_dynamic_normal_t;

/* ---- geometry selection (src/analysis/geometry.rs:24-136, 181-210; input/geometry.rs) ----------
 * Only samples whose bond position lies inside (or, inverted, outside) the shape are accumulated
 * (bond.rs:424-426, uaorder.rs:388-390).  The shape is re-anchored every frame (geometry.rs:192-210). */
typedef enum { GORDER_GEOM_NONE = 0, GORDER_GEOM_CUBOID = 1, GORDER_GEOM_CYLINDER = 2, GORDER_GEOM_SPHERE = 3 } gorder_geom_kind_t;
typedef enum { GORDER_GEOMREF_POINT = 0, GORDER_GEOMREF_BOX_CENTER = 1, GORDER_GEOMREF_GROUP = 2 } gorder_geom_ref_t;
typedef struct {
    uint32_t kind;          /* gorder_geom_kind_t */
    uint32_t invert;
    uint32_t reference;     /* gorder_geom_ref_t: fixed point / box centre / centre of geometry of a group */
    float point[3];
    uint32_t n_group;
    const uint32_t *group;  /* atom indices of group "GeomReference" */
    float xdim[2], ydim[2], zdim[2];   /* cuboid extents relative to the reference; {-inf, +inf} = unbounded */
    float radius;           /* cylinder, sphere */
    float span[2];          /* cylinder: extent along its axis relative to the reference; {-inf, +inf} = unbounded */
    uint32_t orientation;   /* cylinder axis 0/1/2 */
    float structure_box[3]; /* box of the STRUCTURE file: a shape anchored at a fixed point is built (and its
                               anchor wrapped) once, at setup, with that box (geometry.rs:296-311 + :194);
                               box-centre / group references are rebuilt with each frame's box */
} gorder_geometry_t;

/* How P2(cos theta) of calc_sch (mod.rs:78-82) is evaluated.
 * Default (0): from the SQUARED cosine, q = (v.n)^2 / (|v|^2 |n|^2), S = 1.5 q - 0.5: one IEEE division, no square
 *   root, no acos -> cos round trip.  The reference evaluates `angle = acos(clamp(v.n / (|v||n|)))` and then
 *   `angle.cos()` in f32 — mathematically the same number plus <= 2 ulp of rounding noise.  Measured against the
 *   reference pipeline with glibc's acosf / cosf (tools/trig_fidelity.c): 5.9 % of samples move by one 1e-6 tick, never
 *   more, mean shift 2.6e-10 — inside the 1e-6 parity tolerance but NOT bit-identical to the reference.  The squared
 *   form also has half the exponent range (|v| below ~1e-19 nm or above ~1e19 nm is no longer the reference's value).
 * GORDER_FLAG_TRIG_ACOS_COS: evaluate the literal acos -> cos round trip like the reference, with acos and cos computed
 *   BY GLIBC'S ALGORITHMS (restatements of glibc 2.28 - 2.40's acosf and cosf, gm_math.h; rounds 1-3 used own polynomial
 *   kernels, 1.6 % of the ticks one off).  Rust's f32::acos / f32::cos are the platform libm's acosf / cosf: against a
 *   reference built on such a glibc the order sums of this mode are the reference's integers — EQUAL to the oracle's LIBM
 *   mode in the tests, the device's acos / cos / sin compared with the host's over their whole domains
 *   (gorder_hip_selftest_trig).  The price is the f64 polynomial of glibc's cosf: 51 % of the HBM roofline on the
 *   256-lipid membrane where the default runs at 80 %.
 *   The one data-dependent angle of the united-atom construction (unsaturated CH: acos, sin, cos, uaorder.rs:1024-1045)
 *   goes through the same restatements in EVERY mode.
 * GORDER_FLAG_UA_FAST_NORMALISE (united atoms only, opt-in, default off): the virtual-hydrogen construction
 *   (uaorder.rs:947-1104) with tolerance-bounded arithmetic instead of the reference's operation sequence — a / |a| as
 *   a * rsqrt(|a|^2) (integer seed + three Newton steps, relative error ~1e-7 where the reference's two roundings leave
 *   6e-8), no second normalisation of the CH2 rotation axis (uaorder.rs:990-1003), minimum image / wrap as
 *   d - L rint(d / L) and x - L floor(x / L), the ordermap tile of a virtual C-H bond as floor((x - x0) * (1 / bin) + 1/2)
 *   by one fma instead of the rounded IEEE quotient (a position within an ulp or two of the line between two tiles may
 *   land on the other side: 0 of 522 036 on the reference's membrane, 5 of 1 015 808 on the synthetic one).  Every
 *   operation is an IEEE mul / add / fma, restated by the oracle's FAST mode: device and oracle sums stay EQUAL.  Against the reference-faithful (libm) oracle every order parameter
 *   stays within one 1e-6 tick; single samples move more often than with the default (a hydrogen position is
 *   target + 0.109 nm * unit vector rounded to the grid of the target's coordinates, so an ulp in the unit vector
 *   flips that rounding in ~1 % of the components): measured in profiles/r04_ua_fast_fidelity.json.  Not with
 *   GORDER_FLAG_TRIG_ACOS_COS (gorder_hip_create refuses the pair).  The default path is bit-unchanged.
 * GORDER_FLAG_CLUSTER_CUTOFF (GORDER_LEAFLETS_CLUSTERING only, opt-in; any other method: gorder_hip_create refuses): the
 *   clustering definition truncated where f32 cannot see the difference — W_ij = expf(-d_ij^2) where d_ij^2 < 36 nm^2 (the
 *   reference's cut-off distance, 6 nm) and 0 otherwise, d_ij the one 3-D minimum image of the pair also where a box edge is
 *   shorter than 12 nm; expf(-36) = 2.3e-16 adds nothing to a degree that is at least 1.  Everything else (sigma, the
 *   deflation of D^1/2 1, 300 Lanczos steps at most with the same start vector, tolerances, row normalisation, 2-means,
 *   orientation, errors, statistics, priming, frequency, flip, collection) is the method's as stated above.  The group may
 *   hold 2 <= n_membrane <= 131072 atoms.  The heads go into a cell list per assignment frame (cells of at least 6 nm; without
 *   handle_pbc over the heads' bounding box), every row of S v is summed over the cells around its own in a fixed order, and
 *   a frame is spread over the whole device, one launch per Lanczos step and kind of work: a frame's flags and statistics
 *   depend on the frame alone.  Sums are associated in another order than on the dense route, so statistics agree with it
 *   to rounding, not bit for bit.  Without the flag nothing changes, the refusal above 8192 atoms included.
 * GORDER_FLAG_UA_SAMPLES (opt-in): gorder_hip_set_order_histogram and gorder_hip_set_molecule_rows accept united-atom
 *   molecule types, alone or beside bond-based types, and book every virtual C-H sample of the exact hydrogen construction
 *   (k_ua_dist, k_ua_mol; see the two setters).  The two setters then refuse GORDER_FLAG_UA_FAST_NORMALISE: the
 *   tolerance-bounded construction is not covered.  Without the flag nothing changes (the setters refuse united atoms);
 *   with the flag on a handle that calls neither setter nothing changes either: the plan, the kernels queued and
 *   gorder_hip_kernel_time_names are those of a handle without it.  Radial shells, bond correlation and neighbour classes
 *   refuse united atoms with or without the flag. */
typedef enum {
    GORDER_FLAG_TRIG_ACOS_COS = 1u,
    GORDER_FLAG_UA_FAST_NORMALISE = 2u,
    GORDER_FLAG_CLUSTER_CUTOFF = 4u,
    GORDER_FLAG_UA_SAMPLES = 8u
} gorder_flags_t;

typedef struct {
    uint32_t n_atoms;           /* atoms per submitted frame (the decoded "Master" group, common.rs:283-304) */
    uint32_t n_molecule_types;
    const gorder_moltype_t *molecule_types;
    int32_t handle_pbc;         /* 1 = PBC3D (pbc.rs:257-460), 0 = NoPBC (pbc.rs:98-253) */
    float normal[3];            /* static membrane normal (normal.rs:75-87, input/axis.rs:49-58) */
    gorder_leaflets_t leaflets;
    gorder_ordermap_t ordermap;
    int32_t timewise;           /* 1 = keep per-frame partial sums (estimate_error; timewise.rs:130-186) */
    int32_t device;             /* HIP device ordinal */
    uint32_t flags;             /* gorder_flags_t */
    gorder_geometry_t geometry; /* kind = GORDER_GEOM_NONE: every sample counts (geometry.rs:215-284) */
    gorder_dynamic_normal_t dynamic_normal;
} gorder_tables_t;

/* Accumulator slots are numbered in reference iteration order: molecule type major, then bond
 * type (AA/CG) or (united atom, hydrogen) (UA).  n_acc = number of slots.  All result arrays are
 * laid out [3][n_acc] with the leading index 0=total, 1=upper, 2=lower (bond.rs:233-246). */

typedef struct gorder_hip_handle gorder_hip_handle;

/* Development switches: environment variables for A/B measurements and for tests that must reach a fallback path.  None
 * changes results.  They are read once, at gorder_hip_create (and by gorder_hip_plan_tables at its call, which has no
 * handle): the handle keeps what it found, and a variable changed afterwards — before a submit, before gorder_hip_reset,
 * from another thread — no longer affects that handle.  A flag is on when set, non-empty and not "0".  The list
 * (gorder_amd/csrc/switches.h holds it, with the parsing):
 *   GORDER_HIP_KERNEL                  =gather: the L1-gather order kernel instead of LDS staging (plain bond tiles only)
 *   GORDER_HIP_WG_TARGET               =N: the workgroup count the frame chunks of a batch aim at
 *   GORDER_HIP_NPF5                    five prefetch registers in the tiled kernels where four would do
 *   GORDER_HIP_TW_GATHER               per-frame rows through k_bonds_extras instead of k_bonds_tiled_tw
 *   GORDER_HIP_MAPS_GATHER             staged ordermaps through k_bonds_extras instead of k_bonds_tiled_maps
 *   GORDER_HIP_FORCE_DIRECT            every bond a direct item (k_bonds_direct), no tiles
 *   GORDER_HIP_UA_SLOT_WAVES           united-atom waves of one slot instead of 4 slots x 16 molecules
 *   GORDER_HIP_REPLICAS                =N in [1, 1024]: copies of the accumulators the kernels add into (32)
 *   GORDER_HIP_MAP_DIRECT              ordermaps by one atomic per sample even where a slot's map fits LDS
 *   GORDER_HIP_MAP_CHUNKS              =N: chunks of frames of k_map_accumulate
 *   GORDER_HIP_MAP_FOLD_LIMIT          =N in [2, 2^21]: samples a packed ordermap word may hold before it is folded (tests)
 *   GORDER_HIP_NO_SPECULATE            global leaflets by k_leaflets_global first, never one read for leaflets and order parameters
 *   GORDER_HIP_LEAFLETS_GENERIC        the membrane's index list even where the membrane is every atom of the frame in order
 *   GORDER_HIP_SPHERICAL_SLAB          =N: at most N assignment frames per launch of k_leaflets_spherical (tests; only lowers the cap)
 *   GORDER_HIP_CLUSTER_STORED_W        spectral clustering reads W stored once a frame instead of recomputing it
 *   GORDER_HIP_LOCAL_SLAB              =N >= 4: at most N assignment frames per launch group of local leaflets and dynamic normals
 *   GORDER_HIP_LOCAL_ATOMS_ONLY        local leaflets without rows of cells: every candidate atom by atom (k_local_flags)
 *   GORDER_HIP_LOCAL_THREE_KERNELS     the cell list by k_local_bin, k_local_scan and k_local_scatter instead of k_local_build
 *   GORDER_HIP_LOCAL_NO_DECIDE         local leaflets without k_local_decide: the rows kernel for every frame
 *   GORDER_HIP_LOCAL_NO_SUMS           local leaflets without k_local_sums: the cell list for every frame
 *   GORDER_HIP_LOCAL_NO_PRUNE          local leaflets: the exact path for every head, no bound
 *   GORDER_HIP_LOCAL_DECIDE_NOTHING    local leaflets: the bound leaves every head open (a measuring aid)
 *   GORDER_HIP_RADIAL_DIRECT           radial shells by per-sample global atomics even where the table fits LDS
 *   GORDER_HIP_DIST_DIRECT             order distributions by per-sample global atomics even where the table fits LDS
 *   GORDER_HIP_DIST_SAMPLES_PER_WORD   =N in [0, 65536]: samples per table word the chunks of k_bonds_dist are cut for (8)
 *   GORDER_HIP_NB_DIRECT               neighbour classes by per-sample global atomics even where the table fits LDS
 *   GORDER_HIP_NB_SUBRANGE             =N: neighbour classes in sub-ranges of at most N frames
 *   GORDER_HIP_NB_ROW_BYTES            =N: the most bytes the class rows of one sub-range take (1 GiB; tests set it small)
 *   GORDER_HIP_CORR_SUBRANGE           =N: bond reorientation in sub-ranges of at most N frames
 *   GORDER_HIP_CORR_GRID               =chunks: a workgroup of k_bond_corr walks every group of lags of its chunk
 *   GORDER_HIP_MOL_ROWS_STAGING        =N: bytes of the per-molecule rows' device staging (1 GiB; tests set it small)
 *   GORDER_HIP_PREFIX_Q16              =N in [1, 65536]: device decode copies N/65536 of every XTC block, whatever it leads to (tests)
 *   GORDER_HIP_NO_PREFIX               device decode copies whole XTC blocks and learns no part */
int gorder_hip_create(const gorder_tables_t *tables, gorder_hip_handle **out);
void gorder_hip_destroy(gorder_hip_handle *h);

/* number of accumulator slots / ordermap tiles (0 if maps are off) */
uint32_t gorder_hip_n_accumulators(const gorder_hip_handle *h);
uint32_t gorder_hip_ordermap_dims(const gorder_hip_handle *h, uint32_t *nx, uint32_t *ny);

/* Run the launches of this handle on a caller-owned hipStream_t (e.g. PyTorch's current stream).
 * NULL selects the handle's own stream. */
int gorder_hip_set_stream(gorder_hip_handle *h, void *hip_stream);

/* Analyse a batch of frames whose coordinates are ALREADY in HBM.
 *   d_xyz  [n_frames][n_atoms][3] f32 (AoS, exactly as an XTC decoder emits them), 16-byte aligned
 *   d_box  [n_frames][3][3]       f32 box matrix rows (GROMACS/XTC order); must be diagonal
 *   frame_index [n_frames] (HOST) global frame indices = `SystemTopology::frame` (topology/mod.rs:141-144)
 * Asynchronous on the handle's stream; errors raised on the device surface at the next
 * gorder_hip_synchronize / gorder_hip_finish. */
int gorder_hip_submit_device(gorder_hip_handle *h, const float *d_xyz, const float *d_box,
                             const uint64_t *frame_index, uint32_t n_frames);

/* Same, from host memory (pinned or pageable).  Double-buffered: the batch is copied on a copy stream into one of
 * two internal device buffers while the kernels of the previous batch may still be running; the call returns once
 * the copy has left the host buffer (the caller may refill it at once), NOT once the kernels are done.  A host that
 * decodes batch k+1 between two calls therefore overlaps decoding, the PCIe copy and the kernels. */
int gorder_hip_submit_host(gorder_hip_handle *h, const float *xyz, const float *box,
                           const uint64_t *frame_index, uint32_t n_frames);

/* ---- trajectory driver: `read_trajectory` (src/analysis/common.rs:239-342) --------------------------------------
 * Reads one trajectory (XTC, TRR or multi-frame GRO; several files = one concatenated trajectory with the duplicate
 * boundary frames dropped), applies the time window and the step, and feeds the frames to the handle batch by batch
 * through a pipeline: `n_threads` host threads decode batch k+2 into pinned memory while batch k+1 is copied on a
 * copy stream and batch k is analysed (see gorder_amd/csrc/trajectory_driver.h).  The k-th analysed frame gets the
 * global frame index first_frame_index + k * step (SystemTopology::frame, topology/mod.rs:141-144).
 * Returns after the last batch has been analysed (synchronised); results are read with gorder_hip_finish.
 * The first error — of the reader or of the analysis — ends the run (common.rs:248). */
typedef struct {
    const char *const *paths;
    uint32_t n_paths;
    const uint32_t *group;       /* atoms of the file that make up a submitted frame, in order (the "Master" group,
                                    common.rs:283-304); NULL = every atom */
    uint32_t n_group;
    float begin_ps, end_ps;      /* inclusive window on the frame time; end_ps < 0 = to the end */
    uint32_t step;               /* analyse every step-th frame of the window (>= 1) */
    uint32_t n_threads;          /* decoder / copying threads; 0 = the hardware threads, at most 16 */
    uint32_t batch_frames;       /* frames per device batch; 0 = about 128 MB of coordinates (1 GiB with device_decode) */
    uint64_t first_frame_index;  /* 0 for a whole trajectory; a rank that reads a later window passes where it starts */
    uint32_t device_decode;      /* 1: XTC files are decompressed ON THE DEVICE — the host threads only copy the compressed
                                    blocks into pinned memory (gorder_xtc_pack_window), the copy engine moves those
                                    (about a third of the decoded bytes) and gorder_hip_xtc_decode unpacks them (k_xtc_scan:
                                    a wave per frame finds where every 256-atom chunk starts; k_xtc_chunks: a lane per
                                    chunk decodes).  TRR files take the route too, also mixed with XTC files in one run: the
                                    positions of the atoms up to the last analysed one travel as the file holds them
                                    (big-endian f32 or f64) and k_trr_unpack swaps and rounds them.  Same coordinates bit
                                    for bit.  A run with a GRO file in it, or with files of different atom counts, or —
                                    when there is an XTC file in it — of frames so large that fewer than 512 fit a 4-GiB
                                    batch (about 700 000 analysed atoms; an XTC launch takes 0.6 us per atom whatever its
                                    size), uses the host decoder.  When the analysed
                                    atoms end before the frame does, only the leading part of every compressed block the
                                    decoder needs is copied (learned from the first batches; a frame that needs more is
                                    decoded by the host).  0: host decoder threads */
    uint32_t shard_index;        /* SURVEY 8e, contiguous frame shards: with shard_count = n > 1 the call first counts the F frames */
    uint32_t shard_count;        /* the window selects (headers only), then analyses frames [i F / n, (i + 1) F / n) of them,
                                    numbered as in the whole trajectory (first_frame_index + k * step for the k-th selected
                                    frame).  Every rank passes the same trajectory and its own i; gorder_hip_allreduce (or the
                                    host's own reduction) then gives SystemTopology::reduce's result.  With a leaflet frequency
                                    other than every frame a shard that begins between two assignment frames reads the one
                                    frame it depends on itself and primes the handle with it (gorder_hip_prime_leaflets).
                                    0 or 1: the whole trajectory */
    uint32_t reserved;
} gorder_trajectory_t;

typedef struct {
    uint64_t n_frames;               /* frames analysed */
    uint64_t n_batches;
    uint64_t bytes_h2d;              /* coordinate + box bytes copied to the device */
    double seconds_total;            /* wall time of the call */
    double seconds_decode;           /* wall time inside the decoder (overlaps with copies and kernels) */
    double seconds_reader_stalled;   /* the reader waited for a free staging slot: copies / kernels are the bottleneck */
    double seconds_gpu_starved;      /* the submitter waited for a decoded batch: the decoder is the bottleneck */
    uint32_t batch_frames, decoder_threads;   /* what was used */
    uint32_t device_decode;          /* 1: the frames were decompressed (XTC) / unpacked (TRR) on the device */
    uint32_t frames_decoded_by_host; /* device route: frames of which too short a leading part had been copied (see
                                        gorder_xtc_pack_window_ex) and which the host decoded after all */
    uint64_t shard_first, shard_frames_total;   /* with shards: ordinal of this shard's first frame among the F selected; F */
    double seconds_setup;            /* time spent allocating the pinned and device staging buffers (all but the first slot's
                                        share overlaps with reading) */
} gorder_trajectory_stats_t;

int gorder_hip_run_trajectory(gorder_hip_handle *h, const gorder_trajectory_t *trajectory,
                              gorder_trajectory_stats_t *stats /* may be NULL */);
/* The pinned host buffers and device buffers of gorder_hip_run_trajectory (with device_decode: 4 slots of a pinned
 * blob + its device copy + 1 GiB of coordinates) stay with the handle after the call, so that the next trajectory
 * analysed with it does not pay for pinning again (~0.1 s per GB); a run of a different shape (route, batch size)
 * replaces them, gorder_hip_destroy frees them — and so does this call, for a host that wants the memory back. */
void gorder_hip_release_staging(gorder_hip_handle *h);

/* Decompress XTC frames — and unpack TRR frames — on the device (the decoding half of groan_rs' GroupXtcReader and
 * TrrReader, common.rs:283-320):
 * `d_blob` / `d_frames` are device copies of what gorder_xtc_pack_window produced (d_blob 64-byte aligned, blob_bytes >= 64), `d_slot_of`
 * [n_atoms_file] maps a file atom to its place in the output frame or -1 (NULL: every atom, in order), `n_stop` is
 * the number of atoms to go through (gorder_xtc_n_atoms_needed), `d_xyz` [n_frames][n_atoms_out][3] receives exactly
 * what gorder_xtc_next would have written, bit for bit.  Asynchronous on the handle's stream; a corrupt frame is
 * reported as GORDER_ERR_TRAJECTORY_FORMAT by the next synchronising call.  Two kernels: k_xtc_scan (a wave per frame walks the
 * group headers, 64 groups a step, and leaves a checkpoint per 256 atoms) and k_xtc_chunks (a lane per chunk decodes from
 * its checkpoint); a frame table with widths no writer produces (more than 72 bits per atom, a field of more than 32, none at
 * all) is a format error too.  2.5 ms per 3 566 frames of 25 088 atoms.
 * The table may hold TRR frames (bits 2 / 3 of `kind`), alone or beside XTC frames — a trajectory concatenated from files
 * of both formats: those go through k_trr_unpack (byte swap; f64 rounded to nearest even like the host's cast; a thread
 * per four floats of a frame, or per atom with `d_slot_of`), each kernel passes over the frames of the other kind, and a
 * table without frames of a kind queues no kernel for it.  To know which, the call reads the table's `kind` words back in
 * the stream's order first (it waits for what the stream holds so far); the kernels themselves are asynchronous. */
int gorder_hip_xtc_decode(gorder_hip_handle *h, const uint8_t *d_blob, uint64_t blob_bytes,
                          const gorder_xtc_frame_t *d_frames, uint32_t n_frames, uint32_t n_atoms_file,
                          const int32_t *d_slot_of, uint32_t n_stop, float *d_xyz, uint32_t n_atoms_out);

/* Compute (only) the leaflet assignment of ONE frame that precedes a rank's frame range
 * (replaces the cross-thread spin-wait of leaflets.rs:1529-1565). */
int gorder_hip_prime_leaflets(gorder_hip_handle *h, const float *d_xyz, const float *d_box,
                              uint64_t frame_index);

/* Manual assignment (GORDER_LEAFLETS_MANUAL): flags[n_molecules_total] for the assignment frame
 * that applies from `frame_index` on; molecules ordered molecule type major. */
int gorder_hip_set_manual_leaflets(gorder_hip_handle *h, const uint8_t *flags, uint64_t frame_index);

/* ---- whole-trajectory manual tables (`!FromFile` / `!FromMap` leaflets, leaflets.rs:815-858; manual membrane normals from a
 * file, normal.rs:258-298) ---------------------------------------------------------------------------------------------------
 * What gorder_hip_collected_leaflets / _normals of an earlier run (or FATSLiM, an NDX file, ...) gave, handed over ONCE for the
 * whole trajectory: the tables are copied at the call (caller memory is not kept) and stay on the device in packed form — flags
 * at one bit a molecule in u64 words, normals at 12 bytes a molecule.  A submit then only queues work, like every other method:
 * k_replay_flags expands the rows a batch opens into the bytes the order kernels route by, k_replay_normals the batch's normals.
 * gorder_hip_run_trajectory works with both (device-decoded XTC and shards included).
 * The upload is the only call that waits for the stream.  A hipMalloc that fails is GORDER_ERR_DEVICE (the table set before stays).
 * Row lookup, by the global frame_index of every submitted frame:
 *   leaflets  assignment index = frame / leaflets.frequency (0 for frequency 0), leaflets.rs:835-839
 *   normals   row = frame / step; a frame with frame % step != 0 is GORDER_ERR_INVALID_ARGUMENT (normal.rs:276-283 asserts)
 * `first_row` lets a rank upload only its window: row r of the call is row first_row + r of the whole table.  A frame whose row
 * is not in [first_row, first_row + n_rows) is GORDER_ERR_MANUAL_LEAFLET_FRAME / GORDER_ERR_MANUAL_NORMAL_FRAME: found on the
 * host before the batch's first kernel is queued, the batch is refused whole (sums and frame count as before it) and
 * gorder_hip_last_error_frame is the first frame without a row.  (A batch that continues the assignment interval the batch before
 * ended in reads the row the handle carries and needs no row of the window.)
 * n_rows = 0 removes the table.  Setting or removing the leaflet table forgets the carried assignment; gorder_hip_reset keeps
 * both tables and forgets the carried row; gorder_hip_destroy frees them.  While a table is set the one-row / one-batch call
 * of the same kind (gorder_hip_set_manual_leaflets / gorder_hip_set_normals) is GORDER_ERR_INVALID_ARGUMENT.
 * gorder_hip_leaflets returns the most recent row.  GORDER_COLLECT_LEAFLETS: a row is collected for the frames with
 * should_assign(frequency, frame) only — a batch that starts between two assignment frames re-expands its row and appends
 * nothing, as priming does.  Manual normals are never collected (the reference does not store them either). */
/* flags [n_rows][n_molecules_total], Upper=0 / Lower=1 before `flip`, molecule-type-major; needs GORDER_LEAFLETS_MANUAL. */
int gorder_hip_set_manual_leaflet_table(gorder_hip_handle *h, const uint8_t *flags,
                                        uint64_t first_row, uint64_t n_rows);
/* normals [n_rows][n_molecules_total][3], any length (calc_sch normalises); row r belongs to frame (first_row + r) * step.
 * Same precondition as gorder_hip_set_normals (no bond outside an LDS window); replaces the static / dynamic normal of every
 * batch while it is set (the dynamic-normal kernels are not queued). */
int gorder_hip_set_manual_normal_table(gorder_hip_handle *h, const float *normals, uint32_t step,
                                       uint64_t first_row, uint64_t n_rows);

int gorder_hip_synchronize(gorder_hip_handle *h);

/* Synchronise and copy the accumulators out.  Leaves them intact (callers may keep submitting).
 *   sums   [3][n_acc] i64 : sum of round(f64(S) * 1e6)            (order.rs:13-26)
 *   counts [3][n_acc] u64 : n_samples                              (order.rs:178-188)
 * Optional (NULL to skip):
 *   map_sums / map_counts [3][n_acc][nx*ny]  (x-major, y inner; ordermap.rs:100-113)
 * n_frames_analyzed: `total_frames` (topology/mod.rs:141-144). */
int gorder_hip_finish(gorder_hip_handle *h, int64_t *sums, uint64_t *counts, int64_t *map_sums,
                      uint64_t *map_counts, uint64_t *n_frames_analyzed);

/* Per-frame partial sums (timewise.rs:130-186) of the frames submitted so far, in submission order:
 *   tw_sums / tw_counts [n_frames_analyzed][3][n_acc].  Requires tables.timewise = 1. */
int gorder_hip_timewise(gorder_hip_handle *h, int64_t *tw_sums, uint64_t *tw_counts,
                        uint64_t capacity_frames);

/* Error estimates (TimeWiseData::estimate_error, timewise.rs:191-231) and convergence columns (prefix_average,
 * timewise.rs:259-274) made from those rows on the device (kernels_timewise.h): what crosses the link is n_blocks x 3 x n_acc
 * (sum, count) pairs, or one float per (frame, leaflet, group), not the rows.  A group is a list of accumulator slots whose rows
 * are added (a bond, the bonds of a heavy atom, a molecule type, the whole system), in CSR form: group g =
 * slots[group_begin[g] .. group_begin[g + 1]).  Everything is exact integer addition up to one truncating division per value, so
 * the results are those of the host route on gorder_hip_timewise's rows bit for bit, however the frames were batched.
 * All four calls need tables.timewise = 1, wait for the handle's stream like gorder_hip_finish (a device error of the run is
 * returned), leave the rows as they are — a later submit followed by a second call sees the longer history — and keep their
 * scratch in the handle (freed by gorder_hip_destroy); gorder_hip_reset empties the rows, and a call behind it sees none.
 * GORDER_ERR_INVALID_ARGUMENT with a message: tables.timewise = 0, n_blocks < 2, a slot >= n_acc, an empty group, no group,
 * group_begin not ascending.  Zero rows, or total_frames / n_blocks == 0: NaN errors, zero block sums, GORDER_OK.
 * Sharded runs: every rank calls gorder_hip_timewise_blocks with the frame count of the whole analysis and the position of
 * its first row; the outputs are added element by element (they are plain sums) and one rank calls
 * gorder_hip_error_estimate with the merged blocks.  Convergence is chained: rank k's end_* are rank k + 1's carry_*. */
uint32_t gorder_hip_timewise_chunk_frames(void);   /* kTwChunkFrames: rows a workgroup folds; host-only */
uint64_t gorder_hip_timewise_rows(const gorder_hip_handle *h);   /* rows held (frames analysed since create / reset); host-only, does not wait */

/* block sums of this handle's rows against the block grid of the WHOLE analysis:
 * block size = total_frames / n_blocks; this handle's row r sits at position first_position + r; positions from
 * n_blocks * block size on are dropped.  out: [n_blocks][3][n_acc]; partial results of shards add up element by element.
 * *block_size (may be NULL): the block size used. */
int gorder_hip_timewise_blocks(gorder_hip_handle *h, uint32_t n_blocks, uint64_t total_frames,
                               uint64_t first_position, int64_t *block_sums, uint64_t *block_counts,
                               uint64_t *block_size);

/* errors[n_groups][3] (total, upper, lower; NaN where a block holds no sample — without leaflets: upper and lower).
 * block_sums/_counts NULL: this handle's own rows (total_frames = its row count, first_position 0); non-NULL: merged
 * blocks [n_blocks][3][n_acc], uploaded. */
int gorder_hip_error_estimate(gorder_hip_handle *h, uint32_t n_blocks, const uint32_t *group_begin,
                              const uint32_t *slots, uint32_t n_groups, const int64_t *block_sums,
                              const uint64_t *block_counts, float *errors);

/* prefix[n_rows][3][n_groups]: per row the average over the rows up to it (cumulative sum / cumulative count, truncating,
 * / 1e6 as f32; NaN while the cumulative count is 0; no sign flip).  carry_* / end_* [3][n_groups]: the sums and counts
 * before this handle's first row (NULL: zero) and behind its last one (may be NULL).  n_rows = gorder_hip_timewise_rows. */
int gorder_hip_convergence(gorder_hip_handle *h, const uint32_t *group_begin, const uint32_t *slots,
                           uint32_t n_groups, const int64_t *carry_sums, const uint64_t *carry_counts,
                           float *prefix, int64_t *end_sums, uint64_t *end_counts);

/* Leaflet flags of the most recent assignment frame, [n_molecules_total] (Upper=0, Lower=1). */
int gorder_hip_leaflets(gorder_hip_handle *h, uint8_t *flags, uint64_t *assignment_frame);
/* ---- collected history ("Exporting internal data": LeafletClassification::..with_collect, AssignedLeaflets, NormalsStorage,
 * DynamicMembraneNormal::store_normals normal.rs:210-227) --------------------------------------------------------------------
 * gorder_hip_leaflets and gorder_hip_normals give the LAST frame only.  With collection switched on the handle keeps, for
 * every batch however it was cut, one row of leaflet flags per assignment frame (should_assign, leaflets.rs:435-441) and one row
 * of dynamic membrane normals per analysed frame: packed on the device (k_collect_flags: 1 bit a molecule; k_collect_normals:
 * 12 bytes a molecule), copied behind the batch's kernels into pinned host memory the handle owns (chunks of 8 MiB or one batch,
 * never moved, reused after gorder_hip_reset) — a submit stays asynchronous.  A handle that never calls gorder_hip_set_collect
 * queues exactly what it queued before.
 * gorder_hip_set_collect: accepted before the first submit / prime / set_manual_leaflets or right after gorder_hip_reset, else
 *   GORDER_ERR_INVALID_ARGUMENT; GORDER_COLLECT_LEAFLETS needs leaflets.method != NONE (GORDER_LEAFLETS_MANUAL: the rows are
 *   the flags the host handed over, each with its frame_index), GORDER_COLLECT_NORMALS needs dynamic_normal.enabled (static and
 *   manual normals are not stored by the reference either, normal.rs:111-116).
 * gorder_hip_prime_leaflets appends NO row: the primed frame belongs to the shard that analyses it, so the rows of the shards
 *   concatenated by frames[] hold every assignment frame exactly once.
 * gorder_hip_reset clears the rows and keeps the switch; gorder_hip_release_staging keeps the rows.
 * A normal is {NaN, NaN, NaN} where the reference never computed it: AA / CG fetch a molecule's normal after the geometry test
 *   (bond.rs:424-431), so a molecule none of whose bonds lay inside the selection in that frame is NaN; united atoms fetch it
 *   for every molecule before the test (uaorder.rs:412-413): none is NaN.
 * The two readers wait for the handle's stream (a device error of the run is returned as by gorder_hip_synchronize); *n_rows is
 *   always set; GORDER_ERR_INVALID_ARGUMENT if that kind is not being collected or capacity_rows < *n_rows. */
typedef enum { GORDER_COLLECT_LEAFLETS = 1u, GORDER_COLLECT_NORMALS = 2u } gorder_collect_t;
/* Switch collection on (bit set of gorder_collect_t; 0 = off). */
int gorder_hip_set_collect(gorder_hip_handle *h, uint32_t what);
/* Rows collected so far: assignment frames, analysed frames. */
int gorder_hip_collected_counts(gorder_hip_handle *h, uint64_t *n_leaflet_rows, uint64_t *n_normal_rows);
/* flags  [n_rows][n_molecules_total]  Upper=0 / Lower=1, after `flip`, molecules in molecule-type-major order
 * frames [n_rows]                     the assignment frames' global frame indices, ascending in submission order
 * Either pointer may be NULL to skip it; *n_rows is always set. */
int gorder_hip_collected_leaflets(gorder_hip_handle *h, uint8_t *flags, uint64_t *frames,
                                  uint64_t capacity_rows, uint64_t *n_rows);
/* normals [n_rows][n_molecules_total][3]  unit vectors
 * frames  [n_rows]                        global frame indices */
int gorder_hip_collected_normals(gorder_hip_handle *h, float *normals, uint64_t *frames,
                                 uint64_t capacity_rows, uint64_t *n_rows);

/* ---- radial profiles: order sums by distance from the selection's reference, in the same pass -----------------------------
 * A handle whose tables select a cylinder or a sphere can be given ascending radii r[0] < ... < r[n - 1], the last one equal to
 * tables.geometry.radius bit for bit.  Next to everything else it does, it then keeps one (tick sum, sample count) set per shell,
 * accumulator slot and leaflet: shell k holds the samples that pass the tables' selection and have r[k - 1] <= d < r[k]
 * (r[-1] = 0), d the distance the selection itself tests — in the cylinder's plane, or from the sphere's centre.  Membership is
 * the reference's `sqrtf(d2) < r` (groan_rs Cylinder / Sphere ::inside), so selections of increasing radius around one reference
 * are nested exactly, shell k is the integer difference of the selections of radius r[k] and r[k - 1], and the shells add up to
 * what gorder_hip_finish returns.  The kernel is k_bonds_shells (its name in gorder_hip_kernel_time_names / _group); a handle
 * that never calls gorder_hip_set_radial_shells queues exactly what it queued before.
 * gorder_hip_set_radial_shells: accepted before the first submit / prime or right after gorder_hip_reset (the rule of
 *   gorder_hip_set_collect); n_radii = 0 switches the shells off.  GORDER_ERR_INVALID_ARGUMENT, with the reason in
 *   gorder_hip_last_error_message, for radii that are not finite, not > 0, not strictly ascending, more than
 *   GORDER_RADIAL_MAX_SHELLS, or whose last differs from tables.geometry.radius; for a geometry kind other than cylinder or
 *   sphere; for geometry.invert; united-atom molecule types; ordermaps; timewise; dynamic membrane normals; a manual normal table
 *   or normals supplied by gorder_hip_set_normals; GORDER_COLLECT_NORMALS.  A handle with shells in turn refuses
 *   gorder_hip_set_normals and gorder_hip_set_manual_normal_table.  Everything else combines: every leaflet method (manual
 *   tables and GORDER_COLLECT_LEAFLETS included), flip, any frequency, a static normal on an axis or general, both cosine modes,
 *   periodic boundaries or none, all three reference kinds, a cylinder with a finite span and any orientation.
 * gorder_hip_radial_shells: sums / counts [n_shells][3][n_acc], the leading index of a shell total / upper / lower as in
 *   gorder_hip_finish (upper and lower are 0 without leaflets).  Raw integers that add element-wise: shards add them on the host —
 *   gorder_hip_allreduce does NOT carry them.  Waits for the queued batches like gorder_hip_finish (a device error of the run is
 *   returned).  Either array may be NULL; *n_shells is set when the pointer is given (0: shells are off, nothing is written).
 * gorder_hip_reset zeroes the shells; the radii stay.
 * Not covered: united atoms, cuboid selections, per-shell error estimates and convergence.
 * gorder_hip_radial_thresholds (host only, no device): thr[k] = the smallest float whose correctly rounded square root reaches
 *   radii[k], so that `d2 < thr[k]` is exactly `sqrtf(d2) < radii[k]` — what the kernel compares against (0 for a radius that
 *   is not > 0). */
#define GORDER_RADIAL_MAX_SHELLS 32
int gorder_hip_set_radial_shells(gorder_hip_handle *h, const float *radii, uint32_t n_radii);
int gorder_hip_radial_shells(gorder_hip_handle *h, int64_t *sums, uint64_t *counts, uint32_t *n_shells);
int gorder_hip_radial_thresholds(const float *radii, uint32_t n, float *thr);

/* ---- per-molecule order rows: every molecule's own tick sum and sample count, frame by frame ------------------------------
 * Everything above is summed over the molecules of a type.  With molecule rows the handle also keeps, for every analysed frame,
 * every group g of accumulator slots and every molecule m, the sum of the ticks (the x 10^6 fixed point of the order sums) of
 * m's samples whose slot belongs to g, and their number — what Lo/Ld domain detection, annular shells around a protein or a
 * lipid's flip-flop history start from.  The reference has no counterpart.  The rows do not depend on leaflets (a molecule is
 * on one side in a frame: GORDER_COLLECT_LEAFLETS says which); a molecule whose type has no slot in g has count 0; a group may
 * span molecule types; "whole lipid" is the host adding the chain groups — integers add.
 * The order pass then runs as k_bonds_tiled_mol (its name in gorder_hip_kernel_time_names / _group): the tiled kernel with a
 * second output, one 64-bit atomic per (tile, group, molecule) and frame into a device staging block of the batch
 * [frames][n_groups][n_molecules_total] packed words, copied behind the kernel into pinned host memory the handle owns (the
 * chunks of the collected history: 8 MiB or one batch, never moved, reused after gorder_hip_reset) — a submit stays
 * asynchronous.  gorder_hip_finish returns exactly what it returns without the rows.  A handle that never calls
 * gorder_hip_set_molecule_rows queues exactly what it queued before.
 * Memory: 8 bytes per group, molecule and frame of pinned host memory — 256 lipids x 2 groups = 4 KB a frame; 83 333 lipids of
 *   a 1M-bead system x 1 group = 667 KB a frame.  On the device only the staging block of one batch, bounded at 1 GiB: a batch
 *   beyond the bound is walked in frame sub-ranges.  The bound is the environment variable GORDER_HIP_MOL_ROWS_STAGING (bytes),
 *   read once at gorder_hip_create.  No pinned memory: GORDER_ERR_DEVICE.
 * gorder_hip_set_molecule_rows: groups in CSR form over accumulator slots as gorder_hip_error_estimate takes them, disjoint;
 *   n_groups = 0 switches the rows off.  Accepted before the first submit / prime or right after gorder_hip_reset (the rule of
 *   gorder_hip_set_collect).  GORDER_ERR_INVALID_ARGUMENT, with the reason in gorder_hip_last_error_message, for united-atom
 *   molecule types; ordermaps; timewise; a geometry selection; dynamic membrane normals; a manual normal table or normals
 *   supplied by gorder_hip_set_normals; radial shells; a bond that spans more than the LDS window; an empty group; a slot
 *   >= n_acc; a slot in two groups; group_begin not ascending; a group of more than 2047 slots (the int32 sum:
 *   2047 x 10^6 < 2^31).  A handle with rows in turn refuses gorder_hip_set_normals, gorder_hip_set_manual_normal_table and
 *   gorder_hip_set_radial_shells.  Everything else combines: both cosine modes, periodic boundaries or none, a static normal
 *   on an axis or general, every leaflet method, flip, any frequency, GORDER_COLLECT_LEAFLETS, any cut into batches,
 *   gorder_hip_submit_host / _device and gorder_hip_run_trajectory (device decoding included).  Global leaflets are assigned
 *   by their own kernel on this route (no one-read speculation).
 * gorder_hip_molecule_rows_count: rows kept so far; does not wait.
 * gorder_hip_molecule_rows: waits for the handle's stream like gorder_hip_finish (a device error of the run is returned);
 *   sums [n_rows][n_groups][n_molecules_total] int32, counts likewise uint32 (molecule-type-major ids, as the leaflet flags),
 *   frames [n_rows] the global frame indices.  Any pointer may be NULL; capacity_rows < rows: GORDER_ERR_INVALID_ARGUMENT.
 *   Shards concatenate their rows by frames[] on the host, as collected rows; gorder_hip_allreduce does NOT carry them.
 * A batch that ends in an error appends no rows: a submit that fails on the host takes back what it had appended, and once a
 *   device error of the run has surfaced (gorder_hip_synchronize, gorder_hip_finish, gorder_hip_molecule_rows, ...) the rows
 *   of the batch that raised it and of every later batch are gone: the rows end where the run ended.  (Where more than 4096
 *   batches were queued without a synchronisation and the failed one is older than that, the rows are cut at the oldest batch
 *   still known: good rows are lost, none of a failed batch is kept.)  GORDER_HIP_KERNEL=gather does not apply to a handle with
 *   rows.
 * gorder_hip_reset clears the rows and keeps the groups.
 * gorder_hip_molecule_rows_stats: facts of the lane order built at set time — n_runs: (tile, group, molecule) runs = global
 *   atomics per frame; max_runs_per_tile; max_tiles_per_word: how many tiles add into one (group, molecule) word.
 * United atoms (GORDER_FLAG_UA_SAMPLES in tables.flags; without it the setter refuses united-atom molecule types as above):
 *   the united-atom tiles run as k_ua_mol (its name in gorder_hip_kernel_time_names / _group) in place of k_ua_extras — the
 *   exact hydrogen construction and the ticks of k_ua_extras bit for bit, so gorder_hip_finish is unchanged — and every
 *   virtual C-H sample adds into the word of (frame, group of the hydrogen's slot, molecule) of the same staging block; the
 *   hydrogens of one carbon may sit in different groups or in none.  Bond-based types on the same handle keep
 *   k_bonds_tiled_mol; the block is copied out behind both kernels.  The setter then refuses GORDER_FLAG_UA_FAST_NORMALISE
 *   (the message names the fast construction); every other refusal above stands.  gorder_hip_molecule_rows_stats counts the
 *   united-atom tiles' (tile, group, molecule) words in n_runs, max_runs_per_tile and max_tiles_per_word: a molecule's
 *   carbons are spread over the tiles of its group of 64 molecules, so a whole-lipid word is fed by several tiles.
 * Not covered: the fast hydrogen construction; rows together with ordermaps, timewise, geometry selections, dynamic or manual
 *   normals or radial shells; per-molecule error estimates and time averages on the device. */
int gorder_hip_set_molecule_rows(gorder_hip_handle *h, const uint32_t *group_begin, const uint32_t *slots, uint32_t n_groups);
int gorder_hip_molecule_rows_count(gorder_hip_handle *h, uint64_t *n_rows);
int gorder_hip_molecule_rows(gorder_hip_handle *h, int32_t *sums, uint32_t *counts, uint64_t *frames, uint64_t capacity_rows);
int gorder_hip_molecule_rows_stats(gorder_hip_handle *h, uint64_t *n_runs, uint32_t *max_runs_per_tile, uint32_t *max_tiles_per_word);

/* ---- order distributions: sample counts per bin of S, accumulator slot and leaflet, for the whole run ----------------------
 * Everything above reports means.  With an order histogram the handle also counts, in the same pass over the frames, how many
 * samples of every accumulator slot fell into each bin of ascending integer tick edges: bin k holds the samples with
 * edges[k] <= tick < edges[k + 1], tick being the x 10^6 fixed point of the sample's raw S = 1.5 cos^2 - 0.5 (before the
 * sign flip an all-atom report applies).  A sample below edges[0] or at or above the last edge is in no bin.  Edges uniform
 * in S give the distribution of S; edges at 10^6 (1.5 cos^2 theta - 0.5) of uniform angles give the tilt-angle distribution
 * of the bond vectors.  The reference has no counterpart.  The counts are pure integer work: exact, and independent of the
 * launch geometry and the cut into batches.
 * The order pass then runs as k_bonds_dist (its name in gorder_hip_kernel_time_names / _group).  gorder_hip_finish returns
 * exactly what it returns without a histogram.  A handle that never calls gorder_hip_set_order_histogram queues exactly what
 * it queued before.  The counts live on the device: 16 bytes per bin and slot, times up to 256 replicas (at most 64 MiB).
 * The environment variable GORDER_HIP_DIST_DIRECT=1 (read once at gorder_hip_create) takes the kernel's per-sample global
 * atomics where its LDS table would fit.
 * gorder_hip_set_order_histogram: n_edges = 0 switches the histogram off; otherwise 2 <= n_edges <= GORDER_HIST_MAX_BINS + 1
 *   strictly ascending edges.  Accepted before the first submit / prime or right after gorder_hip_reset (the rule of
 *   gorder_hip_set_collect).  GORDER_ERR_INVALID_ARGUMENT, with the reason in gorder_hip_last_error_message, for united-atom
 *   molecule types; ordermaps; timewise; dynamic membrane normals; a manual normal table or normals supplied by
 *   gorder_hip_set_normals; radial shells; molecule rows; a bond that spans more than the LDS window; a plan without bond
 *   samples; bad edges.  A handle with a histogram in turn refuses gorder_hip_set_normals, gorder_hip_set_manual_normal_table,
 *   gorder_hip_set_radial_shells and gorder_hip_set_molecule_rows.  Everything else combines: both cosine modes, periodic
 *   boundaries or none, a static normal on an axis or general, every leaflet method, flip, any frequency,
 *   GORDER_COLLECT_LEAFLETS, any cut into batches, gorder_hip_submit_host / _device and gorder_hip_run_trajectory (device
 *   decoding included), and a geometry selection of any kind, inverted or not: a sample outside the selection is in no bin,
 *   as it is in no sum.  Global leaflets are assigned by their own kernel on this route (no one-read speculation), and
 *   GORDER_HIP_KERNEL=gather does not apply.
 * gorder_hip_order_histogram: waits for the handle's stream like gorder_hip_finish (a device error of the run is returned);
 *   counts [n_bins][3][n_acc], the planes total / upper / lower as in gorder_hip_finish (lower = total - upper; without
 *   leaflets upper and lower are 0); n_bins = n_edges - 1, or 0 with the histogram off (counts is then not written).  Either
 *   pointer may be NULL.  After a batch that ended in an error the counts have the standing of the ordinary accumulators.
 *   Shards add their arrays on the host; gorder_hip_allreduce does NOT carry them.
 * gorder_hip_reset zeroes the counts and keeps the edges.
 * United atoms (GORDER_FLAG_UA_SAMPLES in tables.flags; without it the setter refuses united-atom molecule types as above):
 *   the united-atom tiles run as k_ua_dist (its name in gorder_hip_kernel_time_names / _group) in place of k_ua_extras — the
 *   exact hydrogen construction and the ticks of k_ua_extras bit for bit, a geometry selection tested on the virtual bond's
 *   position as k_ua_extras tests it — and every virtual C-H sample is counted in its bin, into the same replicas as
 *   k_bonds_dist's, which keeps the bond-based types of the same handle.  The LDS table is sized by the widest tile of either
 *   kind (a united-atom tile cut from a small molecule group holds many slots: 62 for six Berger POPC), and
 *   GORDER_HIP_DIST_DIRECT applies to both kernels.  The setter then refuses GORDER_FLAG_UA_FAST_NORMALISE (the message names
 *   the fast construction) and a plan with neither bond nor united-atom samples; every other refusal above stands.
 * gorder_hip_order_histogram_route: which route the histogram set on the handle takes — *direct = 1: per-sample global
 *   atomics (the table of the widest tile does not fit, or GORDER_HIP_DIST_DIRECT), 0: the LDS table —, and *table_bytes,
 *   the size of that table.  Either pointer may be NULL; GORDER_ERR_INVALID_ARGUMENT with the histogram off.
 * Not covered: the fast hydrogen construction; a histogram per frame or per molecule; sums per bin; histograms together with
 *   ordermaps, timewise rows, radial shells, molecule rows, or dynamic or manual normals. */
#define GORDER_HIST_MAX_BINS 256
int gorder_hip_set_order_histogram(gorder_hip_handle *h, const int32_t *edges, uint32_t n_edges);
int gorder_hip_order_histogram(gorder_hip_handle *h, uint64_t *counts, uint32_t *n_bins);
int gorder_hip_order_histogram_route(gorder_hip_handle *h, uint32_t *direct, uint64_t *table_bytes);

/* ---- bond reorientation: the second-rank autocorrelation of every bond vector, in the same pass over the frames ------------
 * Everything above says how ordered a bond is; this says how fast it reorients:  C(lag) = < P2( u(t) . u(t + lag) ) >  over t
 * and the molecules, u the direction of the bond.  Its plateau is S^2, its decay gives correlation times.  The reference has
 * no counterpart.
 * gorder_hip_set_bond_correlation takes 1 .. GORDER_CORR_MAX_LAGS strictly ascending lags, each at most GORDER_CORR_MAX_LAG;
 *   lag 0 is allowed.  The unit of a lag is ANALYSED FRAMES IN SUBMIT ORDER, counted by the handle from its first frame
 *   since gorder_hip_create or gorder_hip_reset — not frame_index.
 * For every bond sample and every analysed frame s with s - lag at or behind that first frame the handle books one tick,
 *   tick = round(10^6 * S),  S = 1.5 q - 0.5,  q = (v_s . v_e)^2 / (|v_s|^2 * n2sq),  e = s - lag,
 *   v = p2 - p1 of that frame under the handle's minimum image (or none), never normalised; the later frame s is the sample,
 *   the earlier frame e plays the membrane normal, n2sq = (x*x + y*y) + z*z of v_e: the arithmetic of a per-molecule manual
 *   normal (gorder_hip_set_normals), operation for operation.  The ticks ALWAYS use this default squared-cosine form, also on
 *   a handle with GORDER_FLAG_TRIG_ACOS_COS: that flag is about reproducing the reference's order parameter, and the
 *   reference has no correlation.
 * A pair is booked on the leaflet its molecule has in the LATER frame s.  Every step is an integer add: the result is exact
 *   and does not depend on the cut into batches, the chunking or the launch geometry.
 * The pass is an additional one behind the batch's leaflet and order kernels (k_bond_units, k_bond_corr in
 *   gorder_hip_kernel_time_names / _group); gorder_hip_finish returns exactly what it returns without it, and a handle that
 *   never calls the setter queues exactly what it queued before.  With the correlation on, global leaflets are assigned by
 *   their own kernel (no one-read speculation).
 * Memory: a ring of max_lag + S frame planes of 16 bytes per bond sample (tiles padded to 256), S the frames of a batch
 *   handled at once; at most 2 GiB.  The ring is allocated at the first submit: S is the largest sub-range that fits, capped
 *   by that batch's length (not below 64), and GORDER_HIP_CORR_SUBRANGE (read once at gorder_hip_create) forces a smaller
 *   one; GORDER_HIP_CORR_GRID=chunks (likewise) takes k_bond_corr's chunk-major grid, same integers.  256 all-atom lipids (16 384 samples) are 262 KB a plane, 1.07 GB at lag 4096; a million coarse-grained bonds are
 *   14.7 MB a plane, about 130 frames of lag.
 * gorder_hip_set_bond_correlation: accepted before the first submit / prime or right after gorder_hip_reset (the rule of
 *   gorder_hip_set_collect); n_lags = 0 switches the correlation off.  GORDER_ERR_INVALID_ARGUMENT, with the reason in
 *   gorder_hip_last_error_message, for united-atom molecule types; a geometry selection (a pair may be half inside); a bond
 *   that spans more than the LDS window; a plan without bond samples; bad lags; a ring that would pass 2 GiB with S = 1 (the
 *   message has the arithmetic).  Everything else combines with it on the same handle: timewise rows, ordermaps, dynamic or
 *   manual normals, every leaflet method, order histograms, molecule rows, both cosine modes of the order parameter.
 * gorder_hip_bond_correlation: waits like gorder_hip_finish (a device error of the run is returned); sums int64
 *   [n_lags][3][n_acc] and counts uint64 [n_lags][3][n_acc], the planes total / upper / lower (lower = total - upper; without
 *   leaflets upper and lower are 0); C of a slot = sums / counts / 10^6.  n_lags = 0 with the correlation off (nothing is
 *   written).  Any pointer may be NULL.  The total count of a lag after F frames is max(0, F - lag) * samples of the slot.
 *   After a batch that ended in an error the arrays have the standing of the ordinary accumulators.
 * gorder_hip_reset zeroes sums and counts, forgets the history and keeps the lags.
 * Pairs across a shard boundary are lost: shards add their arrays on the host (gorder_hip_allreduce does NOT carry them), and
 *   the counts say what is missing.
 * Not covered: united atoms; geometry selections; cross-correlation between different bonds; lags beyond 4096 frames;
 *   per-molecule correlation rows. */
#define GORDER_CORR_MAX_LAGS 64
#define GORDER_CORR_MAX_LAG 4096
int gorder_hip_set_bond_correlation(gorder_hip_handle *h, const uint32_t *lags, uint32_t n_lags);
int gorder_hip_bond_correlation(gorder_hip_handle *h, int64_t *sums, uint64_t *counts, uint32_t *n_lags);

/* ---- order by local composition: neighbour counts per molecule, order sums per class of that count -------------------------
 * Everything above says how ordered a bond is in space, per lipid, as a distribution and in time; this says how a lipid's order
 * depends on what surrounds it — a POPC tail with 0, 1, 2 or 3 cholesterols within a nanometre.  The reference has no
 * counterpart.
 * Per analysed frame and molecule m the handle counts the neighbour atoms q != centres[m] whose distance from the atom
 *   centres[m] is below `radius`: d = x_q - x_c per component in f32; with handle_pbc the minimum image of every component
 *   under the frame's own box; d2 = (dx*dx + dy*dy) + dz*dz; counted where sqrtf(d2) < radius, evaluated as d2 < thr with thr
 *   the value gorder_hip_radial_thresholds gives for the radius.  The distance is three-dimensional and leaflets play no part
 *   in it; an atom is looked at once, at its minimum image.  The class of (frame, m) is min(count, n_classes - 1).
 * Every bond sample of molecule m in that frame is booked, with its ordinary tick, on (class, accumulator slot, leaflet) —
 *   next to everything else the handle does and in the same submit.  Every step is an integer add: the result is exact and
 *   does not depend on the cut into batches, sub-ranges, chunks or the launch geometry, the classes add up to what
 *   gorder_hip_finish returns, and gorder_hip_finish returns exactly what it returns without the feature.  A handle that never
 *   calls the setter queues exactly what it queued before.
 * The order pass then runs as k_neighbour_counts, then k_bonds_classes (their names in gorder_hip_kernel_time_names /
 *   _group).  Global leaflets are assigned by their own kernel on this route (no one-read speculation), and
 *   GORDER_HIP_KERNEL=gather does not apply.  Environment, read once at gorder_hip_create: GORDER_HIP_NB_DIRECT=1 takes
 *   k_bonds_classes' per-sample global atomics where its LDS table would fit; GORDER_HIP_NB_SUBRANGE=n walks a batch in
 *   sub-ranges of n frames; GORDER_HIP_NB_ROW_BYTES=n bounds the class bytes on the device (default 1 GiB).  A batch is walked
 *   in sub-ranges of at most 65 535 frames in any case.
 * An undefined (NaN) x of a centre or a neighbour atom raises GORDER_ERR_UNDEFINED_POSITION for that frame, the atom's index
 *   in gorder_hip_last_error_index (the error key has 17 bits for the molecule, as for the heads of the dynamic normals: the
 *   index is that of the right centre for the first 131 072 molecules; status and frame are right for all).
 * gorder_hip_set_neighbour_classes: centres [n_molecules_total], one atom index per molecule, molecule-type-major (the order of
 *   the leaflet flags); neighbours [n_neighbours] strictly ascending atom indices, 1 .. GORDER_NEIGHBOUR_MAX_ATOMS of them;
 *   radius finite and > 0; 2 <= n_classes <= GORDER_NEIGHBOUR_MAX_CLASSES.  n_neighbours = 0 switches the feature off.
 *   Accepted before the first submit / prime or right after gorder_hip_reset (the rule of gorder_hip_set_collect).
 *   GORDER_ERR_INVALID_ARGUMENT, with the reason in gorder_hip_last_error_message, for united-atom molecule types; direct items
 *   (a bond that spans more than the LDS window); a plan without bond samples; ordermaps; timewise; a geometry selection;
 *   dynamic membrane normals; a manual normal table or normals supplied by gorder_hip_set_normals; radial shells; molecule
 *   rows; an order histogram; an index >= n_atoms; neighbours not strictly ascending or too many; classes out of range; a
 *   bad radius.  A handle with classes in turn refuses gorder_hip_set_normals, gorder_hip_set_manual_normal_table,
 *   gorder_hip_set_radial_shells, gorder_hip_set_molecule_rows and gorder_hip_set_order_histogram.  Everything else combines:
 *   both cosine modes, periodic boundaries or none, a static normal on an axis or general, every leaflet method, flip, any
 *   frequency, any cut into batches, gorder_hip_submit_host / _device and gorder_hip_run_trajectory (device decoding
 *   included).  Bond correlation is an independent pass: allowed, not tested.
 * gorder_hip_neighbour_classes: sums int64 / counts uint64 [n_classes][3][n_acc], the planes total / upper / lower as in
 *   gorder_hip_finish (lower = total - upper; upper and lower are 0 without leaflets).  Waits for the queued batches like
 *   gorder_hip_radial_shells (a device error of the run is returned).  Either array may be NULL; *n_classes is set when the
 *   pointer is given (0: the feature is off, nothing is written).  Shards add the arrays on the host — gorder_hip_allreduce
 *   does NOT carry them.
 * gorder_hip_neighbour_class_rows: a diagnostic like gorder_hip_spherical_stats — the class bytes [n_frames][n_molecules_total]
 *   of the LAST submitted batch (of its last sub-range where the batch exceeds 1 GiB of them; none after gorder_hip_reset).
 *   rows = NULL only returns the sizes; otherwise it waits like gorder_hip_finish.
 * gorder_hip_reset zeroes the class arrays and keeps the setting.
 * Not covered: united atoms; lateral or cylinder distance; a same-leaflet restriction; several neighbour groups at once;
 *   weighting by distance; class rows for a whole run through gorder_hip_set_collect; classes in gorder_hip_allreduce; a cell
 *   list for the count. */
#define GORDER_NEIGHBOUR_MAX_ATOMS 16384
#define GORDER_NEIGHBOUR_MAX_CLASSES 32
int gorder_hip_set_neighbour_classes(gorder_hip_handle *h, const uint32_t *centres, const uint32_t *neighbours, uint32_t n_neighbours,
                                     float radius, uint32_t n_classes);
int gorder_hip_neighbour_classes(gorder_hip_handle *h, int64_t *sums, uint64_t *counts, uint32_t *n_classes);
int gorder_hip_neighbour_class_rows(gorder_hip_handle *h, uint8_t *rows, uint32_t *n_frames, uint32_t *n_mol);

/* Signed distances (nm) behind those flags, [n_molecules_total] (leaflets.rs:725, 796).  GORDER_LEAFLETS_SPHERICAL: each
 * molecule's head-centre distance (nm, non-negative) in the last assignment frame. */
int gorder_hip_leaflet_distances(gorder_hip_handle *h, float *distances);
/* GORDER_LEAFLETS_SPHERICAL, the most recent assignment frame: out[0..2] centre of the group (x, y, z); out[3..7] the fitted
 * mixture — weight_a, mean_a, var_a, mean_b, var_b (GmmParams, spherical_clustering.rs:80-97); out[8] final average
 * log-likelihood; out[9] EM iterations run (E-steps, at most 50); out[10] group atoms labelled outer (upper, before `flip`);
 * out[11] reserved, 0.  GORDER_ERR_INVALID_ARGUMENT for other methods or before any assignment.  Waits for the stream. */
int gorder_hip_spherical_stats(gorder_hip_handle *h, float out[12]);
/* GORDER_LEAFLETS_CLUSTERING, the most recent assignment frame: out[0..2] the eigenvalues 2, 3, 4 of L as the solver sees them
 * (1 - Ritz value; NaN where the group is too small to have one); out[3] Lanczos steps used; out[4] 2-means rounds (label
 * passes, the one that found no change included); out[5], out[6] atoms in 2-means cluster 0 and 1; out[7], out[8] atoms in the
 * upper and the lower leaflet (before `flip`); out[9], out[10] o_up, o_lo: the share of cluster 0 that was upper / lower in the
 * previous assignment frame (NaN for frame 0); out[11] reserved, 0.  gorder_hip_leaflet_distances gives each molecule's first
 * embedding coordinate (v2 after row normalisation, sign: the group's first atom is not negative).
 * gorder_hip_prime_leaflets: frame 0 gives the ab-initio orientation, a later frame is matched against the clusters the handle
 * holds — a shard primes frame 0, then the last assignment frame before its range; a later assignment frame with nothing held
 * is GORDER_ERR_LEAFLETS_NOT_PRIMED; gorder_hip_reset forgets the held clusters.
 * GORDER_ERR_INVALID_ARGUMENT for other methods or before any assignment.  Waits for the stream. */
int gorder_hip_clustering_stats(gorder_hip_handle *h, float out[12]);

/* Manual membrane normals (MembraneNormal::Manual, ManualMembraneNormal::get_normal, normal.rs:266-300): the host
 * resolves the normals file and hands over, before a submit call, one vector per frame of that batch and per
 * molecule — normals [n_frames][n_molecules_total][3] (host memory, copied; any length, calc_sch normalises).
 * They replace the static / dynamic normal for exactly the next gorder_hip_submit_* call, whose n_frames must
 * match. */
int gorder_hip_set_normals(gorder_hip_handle *h, const float *normals, uint32_t n_frames);

/* Dynamic membrane normals of the LAST submitted frame: normals [n_molecules_total][3] (unit vectors; NaN
 * for a molecule whose cloud had fewer than 3 points), n_points [n_molecules_total] the cloud sizes
 * (what NormalsStorage keeps per frame, normal.rs:460-520).  Requires tables.dynamic_normal.enabled. */
int gorder_hip_normals(gorder_hip_handle *h, float *normals, uint32_t *n_points);

/* Device pointer + element count of the packed 64-bit accumulator block, n_u64 = 4 * n_acc + 1 words:
 *   { i64 sum_total[n_acc], i64 sum_upper[n_acc], u64 count_total[n_acc], u64 count_upper[n_acc], u64 total_frames }
 * (lower = total - upper: every sample is upper or lower, bond.rs:199-213; gorder_hip_finish derives it), so that
 * a host can issue ONE RCCL all-reduce (ncclInt64 / ncclSum) over it — the multi-GPU form of
 * SystemTopology::reduce (topology/mod.rs:256-272).  Ordermaps are NOT part of the block: see
 * gorder_hip_export_maps / gorder_hip_allreduce. */
int gorder_hip_accumulators_device(gorder_hip_handle *h, void **d_ptr, uint64_t *n_u64);

/* ---- multi-GPU reduce inside the library (for hosts without a collective library of their own) -------------------
 * gorder_hip_allreduce sums, in place and across the ranks of an initialised RCCL communicator (`ncclComm_t`, passed
 * as void *), everything SystemTopology::add sums (topology/mod.rs:236-254): the packed accumulator block (order sums,
 * counts, total_frames) and, with ordermaps, the maps — ONE group of ncclAllReduce(ncclInt64, ncclSum) calls on the
 * handle's stream, over xGMI on an MI355X node.  Call it once, after the rank's last batch; every rank then reads the
 * whole-trajectory result with gorder_hip_finish.  Per-frame timewise rows and leaflet flags are per-rank data and are
 * not touched (the host concatenates them by frame index).  RCCL is bound at the first call (librccl.so.1).
 * The communicator can come from the host's own RCCL calls or from the two helpers below:
 *   rank 0: gorder_hip_comm_unique_id(id) -> the host ships the 128 bytes to the other ranks (any channel) ->
 *   every rank: gorder_hip_comm_create(handle, id, n_ranks, rank, &comm) on its handle's device. */
int gorder_hip_comm_unique_id(uint8_t id[128]);
int gorder_hip_comm_create(gorder_hip_handle *h, const uint8_t id[128], int n_ranks, int rank, void **comm_out);
void gorder_hip_comm_destroy(void *comm);
int gorder_hip_allreduce(gorder_hip_handle *h, void *nccl_comm);

/* Forget everything accumulated so far (sums, counts, maps, timewise rows, frame count, leaflet carry, error
 * state): the handle is a fresh `SystemTopology` on the same tables.  Stream-ordered. */
int gorder_hip_reset(gorder_hip_handle *h);

/* Ordermaps for the same reduction: copies the folded maps, i64 sums and u64 counts laid out
 * [3][n_acc][nx*ny] (n_u64 = 3 * n_acc * nx * ny words each, see gorder_hip_ordermap_dims), into caller-owned
 * device buffers (e.g. two torch.int64 tensors) that the host all-reduces like the accumulator block
 * (Map::add, ordermap.rs:116-138).  Stream-ordered after everything submitted so far; synchronises. */
int gorder_hip_export_maps(gorder_hip_handle *h, void *d_sums, void *d_counts, uint64_t n_u64);

/* Ordermaps finished on the device (kernels_ordermap.h): the maps the reference writes into its ordermap directory
 * (ResultsConverter::convert_ordermap, converter.rs:226-256), made from the raw tile sums where they lie, so that one float per
 * (group, plane, tile) crosses the link instead of 16 bytes per (slot, plane, tile).  A group is a list of accumulator slots
 * whose tiles are added (a bond, the bonds of a heavy atom, a molecule type, the whole system) in the CSR form of
 * gorder_hip_error_estimate: group g = slots[group_begin[g] .. group_begin[g + 1]).  A tile's value (ordermap_final.h):
 *   count < min_samples -> NaN;  v = (float)((double)sum / 1e6);  v = v / (float)count;  negate != 0 -> -v
 * — the f32 division of the converter, not the truncating i64 division of calc_order that the order parameters take; the
 * sums before it are exact integers, so the result is the host's on gorder_hip_finish's maps bit for bit.  negate: 1 for
 * all-atom and united-atom analyses (they report -S; a zero sum then gives -0.0 as in the reference), 0 for coarse-grained.
 * maps: host, [n_groups][3][nx*ny] (total, upper, lower; tiles x-major as in gorder_hip_finish); without leaflets the upper and
 * lower planes are NaN.
 * d_sums / d_counts NULL: the handle's own maps — after gorder_hip_allreduce those of the whole analysis.  Non-NULL: device
 * arrays in gorder_hip_export_maps' layout, complete when the call is made (e.g. the exported maps of several ranks added by the
 * host's collective); n_u64 must then be 3 * n_acc * nx * ny.
 * The call waits for the handle's stream like gorder_hip_finish (a device error of the run is returned), leaves the maps as
 * they are — a later submit followed by a second call sees the longer history — and keeps its scratch in the handle (freed
 * by gorder_hip_destroy).  After gorder_hip_reset, or before any frame, every tile is NaN.
 * GORDER_ERR_INVALID_ARGUMENT with a message: ordermaps off, min_samples == 0, no group, an empty group, a slot >= n_acc,
 * group_begin not ascending, only one of d_sums / d_counts, a wrong n_u64, a NULL output. */
int gorder_hip_ordermaps(gorder_hip_handle *h, const uint32_t *group_begin, const uint32_t *slots, uint32_t n_groups,
                         uint32_t min_samples, uint32_t negate, const void *d_sums, const void *d_counts,
                         uint64_t n_u64, float *maps);

/* Make the handle accumulate into caller-owned device memory (>= n_u64 words, 8-byte aligned; e.g.
 * a torch.int64 tensor that the host then hands to torch.distributed.all_reduce = RCCL).  The
 * current contents of the handle's accumulators are copied over. */
int gorder_hip_bind_accumulators(gorder_hip_handle *h, void *d_ptr, uint64_t n_u64);

/* Payload of the last UndefinedPosition / InvalidLocalMembraneCenter error (atom index). */
uint64_t gorder_hip_last_error_index(const gorder_hip_handle *h);
/* The frame (SystemTopology::frame, i.e. the frame_index the host passed) in which the last device error was raised:
 * the first error of the run in trajectory order — batches in the order of submission, inside a batch the order of the
 * reference's sequential walk (common.rs:201-235, 248). */
uint64_t gorder_hip_last_error_frame(const gorder_hip_handle *h);
const char *gorder_hip_last_error_message(const gorder_hip_handle *h);
const char *gorder_hip_strerror(int status);

/* Device time of the submits since the last call with reset != 0 (ms, HIP events on the stream the handle launches on) and
 * their number.  The first call switches the timing on; submits before it are not timed.  A submit is timed as a chain of
 * segments, one per kernel group it queues — the leaflet kernels ("k_leaflets_global_contig"; "k_leaflets_spherical";
 * "k_cluster_degrees", "k_cluster_lanczos", "k_cluster_embed", "k_cluster_orient" per slab of frames (with
 * GORDER_FLAG_CLUSTER_CUTOFF: "k_clcut_cells", "k_clcut_lanczos", "k_clcut_embed", "k_cluster_orient"); "k_local_build",
 * "k_local_rowprefix", "k_local_flags_rows", "k_local_flags_todo" per 256-frame slab; ...), "k_dyn_cov + k_dyn_eigen",
 * "k_geom_shapes", the order kernels ("k_bonds_tiled", "k_ua_extras", "k_bonds_tiled_maps", ...), "k_map_accumulate",
 * "k_bonds_direct", with manual tables "k_replay_flags" and "k_replay_normals" (ahead of the order kernels), with collection
 * "k_collect_flags" and "k_collect_normals" (the copy to the host included), "k_batch_end", and for gorder_hip_xtc_decode on a
 * table with TRR frames "k_trr_unpack" —; *ms is the sum over all segments, i.e. the WHOLE step on the device. */
int gorder_hip_kernel_time(gorder_hip_handle *h, double *ms, uint64_t *launches, int reset);
/* Group `index` of the same measurement (in order of first appearance since the last reset): its name, the device time
 * of its segments and their number.  GORDER_ERR_INVALID_ARGUMENT past the last group.  The times of all groups add up to
 * gorder_hip_kernel_time's *ms.  Call before gorder_hip_kernel_time(..., reset = 1). */
int gorder_hip_kernel_time_group(gorder_hip_handle *h, uint32_t index, const char **name, double *ms, uint64_t *segments);
/* The group names since the last reset joined by " + ", e.g. "k_bonds_tiled + k_batch_end" ("" before the first timed
 * submit); valid until the next submit or reset. */
const char *gorder_hip_kernel_time_names(const gorder_hip_handle *h);

/* Introspection for tests / DESIGN.md: how the bond table was tiled. */
typedef struct {
    uint32_t n_tiles;
    uint32_t block_threads;
    uint32_t max_window_atoms;
    uint32_t n_direct_items;     /* samples that did not fit an LDS window (direct-gather kernel) */
    uint32_t frames_per_stage;
    uint32_t lds_bytes;
    uint32_t map_staged;         /* 1: ordermap samples go through the staging buffer + k_map_accumulate (LDS) */
    uint32_t map_lds_bytes;      /* packed map of one accumulator slot (x2 with leaflets) = k_map_accumulate's LDS */
    uint32_t leaflets_one_read;  /* 1: global leaflets can be assigned from the order kernel's own read of the frame (the
                                  * membrane group is one range of atoms the tiles' windows cover, every head in it) */
} gorder_hip_plan_t;
int gorder_hip_plan(const gorder_hip_handle *h, gorder_hip_plan_t *plan);
/* Same, without touching a device (host logic only); *selfcheck = 0 when every sample of the
 * tables is covered exactly once by the plan. */
int gorder_hip_plan_tables(const gorder_tables_t *tables, gorder_hip_plan_t *plan, int *selfcheck);

/* Global leaflets assigned every frame, nothing but the order parameters asked for: from the second batch on the library
 * reads every frame ONCE — the order kernel routes each molecule by the last assignment and sums the membrane group's
 * normal coordinate on the way, the exact centres follow from the sums, and the few (frame, molecule) pairs whose side
 * was mispredicted are moved afterwards (GORDER_HIP_NO_SPECULATE=1 keeps the two-kernel path; so does a
 * membrane group that is not one range of atoms the tiles can cover).  Results are the two-kernel path's.
 * out[0] = batches that ran this way, out[1] = mispredicted (frame, molecule) pairs moved, out[2] = frames whose centre
 * the sums could not vouch for (they took the exact kernel), out[3] = 1 while the handle still speculates (it stops
 * when a batch leaves more than 1/8 of its frames to the exact kernel or mispredicts more than 1/16 of its pairs).
 * Waits for the handle's stream. */
int gorder_hip_speculation_stats(gorder_hip_handle *h, uint64_t out[4]);

/* Local leaflets in a periodic box: a kernel of its own (k_local_decide) first tries every head against a bound on what the
 * atoms in the ring of cells the cylinder cuts can change about its side — from per-cell sums made without sorting the
 * atoms (k_local_sums) —, and a frame whose heads it all decides skips the cell list and the pass that looks at those
 * atoms.  A submit that finds the majority of its frames left open — a membrane
 * that undulates by more than the water around it allows — sends the next 16 submits down the atom-by-atom pass alone.
 * The sides are the reference's either way.  (Device memory: a handle with local leaflets holds up to 4 GiB of cell-list
 * scratch — 2 048 assignment frames a launch group, fewer for membranes that need more than 2 MB a frame;
 * GORDER_HIP_LOCAL_SLAB=n caps the frames, at least 4; it sizes the launch groups of dynamic normals as well.
 * GORDER_HIP_SPHERICAL_SLAB=n, at least 1, does the same for spherical clustering of a group beyond 16 384 atoms, whose
 * scratch rows hold at most 64 MiB and 4 096 assignment frames a launch: it only lowers that cap.  Both are read at
 * gorder_hip_create and change no result.)  out[0] = submits that ran the bound kernel, out[1] = submits that paused it,
 * out[2] / out[3] = frames left open / frames seen in the last report read back.  (GORDER_HIP_LOCAL_NO_DECIDE=1: never.)
 * Waits for the handle's stream. */
int gorder_hip_local_decide_stats(gorder_hip_handle *h, uint64_t out[4]);

/* Diagnostic: the kernels replace the IEEE division and square root by their Newton cores inside guarded operand
 * ranges (gm_div_core / gm_sqrt_core in gm_math.h; DESIGN.md, K1 arithmetic).  This runs both forms on `n` pseudo-random
 * operand sets on the device — divisors and radicands log-uniform over the guarded range [2^-40, 2^40], numerators of
 * either sign from 2^-100 to 2^60 and exact zeros — and returns how many results differ in any bit:
 * mismatches[0] division, mismatches[1] square root and the acos kernel with the cores inside against the same kernel
 * with IEEE operations (arguments over all of [-1, 1]).  Both must be 0. */
int gorder_hip_selftest_arithmetic(int device, uint64_t n, uint64_t seed, uint64_t mismatches[2]);
/* Diagnostic: the device's acos (fn 0; 1: with the division / square-root cores inside), cos (2) and sin (3) — restatements
 * of glibc's acosf / cosf / sinf algorithms, gm_math.h — of the `n` floats with bit patterns first_bits + i * stride, into
 * the HOST array `out`: to be compared with the host's libm (tests/test_parity_gpu.py does, over all of [-1, 1] and
 * [0, pi] in strides). */
int gorder_hip_selftest_trig(int device, int fn, uint32_t first_bits, uint32_t stride, uint32_t n, float *out);
/* Diagnostic: ONE workgroup of `block` threads (a multiple of 64, at most 1024) runs every wave and block reduction of the
 * kernels (csrc/wave_ops.h) on one value per thread of the HOST arrays f64, f32, u32 [block] and returns what every lane
 * holds afterwards: out_*[row * block + thread], to be compared bit for bit with the literal restatement of the two
 * orders in tests/wave_ops_ref.py.  Rows (a "row sum" is defined in lane 15 of each 16 lanes, a "rows" total in lane 63):
 *   out_f64: 0 row sum, 1 + rows to wave, 2 wave sum (rows), 3 wave scan (rows), 4 wave sum (butterfly), 5 block sum of x,
 *            6 block sum of 3 x (the same call), 7 lane 47's value, 8 / 9 sums of x and 3 x by the four-quantity butterfly
 *   out_f32: 0 row sum, 1 + rows to wave, 2 wave sum (rows), 3 / 4 wave min / max (rows), 5 / 6 min / max (butterfly),
 *            7 / 8 block min / max, 9 row_shr:1 or own value, 10 row_bcast:31 into rows 2, 3 or zero, 11 lane 47's value,
 *            12 / 13 min / max by the four-quantity butterfly, 14 / 15 by the three-quantity one
 *   out_u32: 0 row sum, 1 + rows to wave, 2 wave sum (rows), 3 wave scan (rows), 4 wave scan (shuffles), 5 or
 *            (butterfly), 6 max (butterfly), 7 wave sum (rows) as int, 8 lane 47's value
 *   out_finfo [9]: a frame's record (key of min f32, key of max f32, or of u32, 2) with every flag kept, the same with
 *            bit 0 only, and the flags thread 0 is left with; finfo_empty != 0: no thread has a value (min > max). */
#define GORDER_WAVE_OPS_F64_ROWS 10
#define GORDER_WAVE_OPS_F32_ROWS 16
#define GORDER_WAVE_OPS_U32_ROWS 9
#define GORDER_WAVE_OPS_FINFO_WORDS 9
int gorder_hip_selftest_wave_ops(int device, uint32_t block, const double *f64, const float *f32, const uint32_t *u32,
                                 int finfo_empty, double *out_f64, float *out_f32, uint32_t *out_u32, uint32_t *out_finfo);

#ifdef __cplusplus
}
#endif
#endif /* GORDER_HIP_H */
