"""ctypes view of include/gorder_hip.h plus a thin engine wrapper.

Python is harness only (tests, bench, multi-GPU launcher): the product is the C-ABI library
``gorder_amd/libgorder_hip.so`` built from ``gorder_amd/csrc`` (hand-written HIP for gfx950).
There is NO CPU fallback here: if the library or a GPU is missing every call raises.

The table classes mirror what gorder's ``SystemTopology`` holds for this path
(/root/reference/src/analysis/topology/mod.rs:34-65, topology/bond.rs:220-246,
leaflets.rs:575-590, 744-775).
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GORDER_HIP_LIB") or os.path.join(_HERE, "libgorder_hip.so")   # env: A/B builds

# ---- status codes (gorder_status_t) ---------------------------------------------------------
OK = 0
ERR_UNDEFINED_BOX = 1
ERR_NOT_ORTHOGONAL_BOX = 2
ERR_ZERO_BOX = 3
ERR_UNDEFINED_POSITION = 4
ERR_INVALID_GLOBAL_MEMBRANE_CENTER = 5
ERR_INVALID_LOCAL_MEMBRANE_CENTER = 6
ERR_DYNAMIC_NORMAL = 7
ERR_MANUAL_LEAFLET_FRAME = 8     # a frame has no row in the manual leaflet table (HipEngine.set_manual_leaflet_table)
ERR_MANUAL_NORMAL_FRAME = 9      # a frame has no row in the manual normal table (HipEngine.set_manual_normal_table)
ERR_INVALID_ARGUMENT = 100
ERR_DEVICE = 101
ERR_NO_DEVICE = 102
ERR_BOX_RANGE = 103
ERR_LEAFLETS_NOT_PRIMED = 104
ERR_OVERFLOW = 105
ERR_TRAJECTORY_FORMAT = 106
ERR_CLUSTERING = 107         # spherical / spectral clustering: a distance of an assignment frame is not finite
ERR_CLUSTER_MATCH = 108      # spectral clustering: the clusters match neither leaflet of the previous assignment frame

LEAFLETS_NONE, LEAFLETS_GLOBAL, LEAFLETS_LOCAL, LEAFLETS_INDIVIDUAL, LEAFLETS_MANUAL, LEAFLETS_SPHERICAL = range(6)
LEAFLETS_CLUSTERING = 6      # spectral clustering (include/gorder_hip.h): membranes of any shape
COLLECT_LEAFLETS, COLLECT_NORMALS = 1, 2   # gorder_collect_t: what HipEngine.set_collect keeps of every frame
FLAG_TRIG_ACOS_COS = 1
FLAG_UA_FAST_NORMALISE = 2      # united atoms: tolerance-bounded hydrogen construction (include/gorder_hip.h)
FLAG_CLUSTER_CUTOFF = 4         # LEAFLETS_CLUSTERING: 6 nm cut-off route for groups of up to 131072 atoms (include/gorder_hip.h)
FLAG_UA_SAMPLES = 8             # set_order_histogram / set_molecule_rows accept united-atom molecule types (include/gorder_hip.h)
UA_CH1_SAT, UA_CH2, UA_CH3, UA_CH1_UNSAT = 1, 2, 3, 4
UA_N_H = {UA_CH1_SAT: 1, UA_CH2: 2, UA_CH3: 3, UA_CH1_UNSAT: 1}

_u32p = C.POINTER(C.c_uint32)


class CLeaflets(C.Structure):
    _fields_ = [("method", C.c_uint32), ("normal_dim", C.c_uint32), ("frequency", C.c_uint32),
                ("flip", C.c_uint32), ("radius", C.c_float), ("n_membrane", C.c_uint32),
                ("membrane", _u32p)]


class COrderMap(C.Structure):
    _fields_ = [("enabled", C.c_uint32), ("plane", C.c_uint32), ("span_x", C.c_float * 2),
                ("span_y", C.c_float * 2), ("bin", C.c_float * 2)]


class CUaAtom(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("indices", _u32p)]


class CMolType(C.Structure):
    _fields_ = [("n_molecules", C.c_uint32), ("n_bond_types", C.c_uint32), ("bonds", _u32p),
                ("n_ua_atoms", C.c_uint32), ("ua_atoms", C.POINTER(CUaAtom)), ("heads", _u32p),
                ("n_methyls", C.c_uint32), ("methyls", _u32p), ("normal_heads", _u32p)]


class CDynamicNormal(C.Structure):
    _fields_ = [("enabled", C.c_uint32), ("radius", C.c_float), ("n_cloud", C.c_uint32), ("cloud", _u32p)]


class CGeometry(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("invert", C.c_uint32), ("reference", C.c_uint32), ("point", C.c_float * 3),
                ("n_group", C.c_uint32), ("group", _u32p), ("xdim", C.c_float * 2), ("ydim", C.c_float * 2),
                ("zdim", C.c_float * 2), ("radius", C.c_float), ("span", C.c_float * 2), ("orientation", C.c_uint32),
                ("structure_box", C.c_float * 3)]


class CTables(C.Structure):
    _fields_ = [("n_atoms", C.c_uint32), ("n_molecule_types", C.c_uint32),
                ("molecule_types", C.POINTER(CMolType)), ("handle_pbc", C.c_int32),
                ("normal", C.c_float * 3), ("leaflets", CLeaflets), ("ordermap", COrderMap),
                ("timewise", C.c_int32), ("device", C.c_int32), ("flags", C.c_uint32), ("geometry", CGeometry),
                ("dynamic_normal", CDynamicNormal)]


class CTrajectory(C.Structure):
    _fields_ = [("paths", C.POINTER(C.c_char_p)), ("n_paths", C.c_uint32), ("group", _u32p), ("n_group", C.c_uint32),
                ("begin_ps", C.c_float), ("end_ps", C.c_float), ("step", C.c_uint32), ("n_threads", C.c_uint32),
                ("batch_frames", C.c_uint32), ("first_frame_index", C.c_uint64), ("device_decode", C.c_uint32),
                ("shard_index", C.c_uint32), ("shard_count", C.c_uint32), ("reserved", C.c_uint32)]


class CTrajectoryStats(C.Structure):
    _fields_ = [("n_frames", C.c_uint64), ("n_batches", C.c_uint64), ("bytes_h2d", C.c_uint64),
                ("seconds_total", C.c_double), ("seconds_decode", C.c_double), ("seconds_reader_stalled", C.c_double),
                ("seconds_gpu_starved", C.c_double), ("batch_frames", C.c_uint32), ("decoder_threads", C.c_uint32),
                ("device_decode", C.c_uint32), ("frames_decoded_by_host", C.c_uint32), ("shard_first", C.c_uint64),
                ("shard_frames_total", C.c_uint64), ("seconds_setup", C.c_double)]


class CXtcFrame(C.Structure):
    """gorder_xtc_frame_t (include/gorder_xtc.h): one still-compressed XTC frame, or the big-endian positions of a TRR
    frame (kind 4: f32, 8: f64), for the device decoder."""
    _fields_ = [("offset", C.c_uint64), ("recip1", C.c_uint64), ("recip2", C.c_uint64), ("n_bytes", C.c_uint32),
                ("kind", C.c_uint32), ("minint", C.c_int32 * 3), ("sizeint", C.c_uint32 * 3), ("smallidx", C.c_int32),
                ("inv_precision", C.c_float), ("bitsize", C.c_uint32), ("bitsizeint", C.c_uint32)]


class CPlan(C.Structure):
    _fields_ = [("n_tiles", C.c_uint32), ("block_threads", C.c_uint32),
                ("max_window_atoms", C.c_uint32), ("n_direct_items", C.c_uint32),
                ("frames_per_stage", C.c_uint32), ("lds_bytes", C.c_uint32),
                ("map_staged", C.c_uint32), ("map_lds_bytes", C.c_uint32), ("leaflets_one_read", C.c_uint32)]


# ---- python-side description of the tables ----------------------------------------------------
def _u32(a, shape=None) -> Optional[np.ndarray]:
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.uint32)
    if shape is not None:
        a = a.reshape(shape)
    return a


def _ptr(a: Optional[np.ndarray]):
    if a is None or a.size == 0:
        return _u32p()
    return a.ctypes.data_as(_u32p)


@dataclass
class MolType:
    """One molecule type (topology/molecule.rs:146-169) reduced to its index tables."""
    n_molecules: int
    bonds: Optional[np.ndarray] = None        # [n_bond_types, n_molecules, 2] uint32
    ua_atoms: List[tuple] = field(default_factory=list)   # [(kind, indices[n_molecules, 4])]
    heads: Optional[np.ndarray] = None        # [n_molecules]
    methyls: Optional[np.ndarray] = None      # [n_molecules, n_methyls]
    name: str = ""
    normal_heads: Optional[np.ndarray] = None  # [n_molecules] (dynamic membrane normals)

    @property
    def n_bond_types(self) -> int:
        return 0 if self.bonds is None else int(np.asarray(self.bonds).shape[0])

    @property
    def n_slots(self) -> int:
        return self.n_bond_types + sum(UA_N_H[int(k)] for k, _ in self.ua_atoms)


@dataclass
class Leaflets:
    method: int = LEAFLETS_NONE
    normal_dim: int = 2
    frequency: int = 1      # 0 = once; REAL frequency (input frequency * step)
    flip: bool = False
    radius: float = 0.0
    membrane: Optional[np.ndarray] = None     # Global / Local: group "Membrane"; Spherical / Clustering: group "ClusterHeads"


@dataclass
class OrderMap:
    enabled: bool = False
    plane: int = 0
    span_x: Sequence[float] = (0.0, 0.0)
    span_y: Sequence[float] = (0.0, 0.0)
    bin: Sequence[float] = (0.1, 0.1)


GEOM_NONE, GEOM_CUBOID, GEOM_CYLINDER, GEOM_SPHERE = range(4)
GEOMREF_POINT, GEOMREF_BOX_CENTER, GEOMREF_GROUP = range(3)
_INF = float("inf")


@dataclass
class Geometry:
    """input/geometry.rs: cuboid / cylinder / sphere relative to a point, the box centre or a group centre."""
    kind: int = GEOM_NONE
    invert: bool = False
    reference: int = GEOMREF_POINT
    point: Sequence[float] = (0.0, 0.0, 0.0)
    group: Optional[np.ndarray] = None
    xdim: Sequence[float] = (-_INF, _INF)
    ydim: Sequence[float] = (-_INF, _INF)
    zdim: Sequence[float] = (-_INF, _INF)
    radius: float = 0.0
    span: Sequence[float] = (-_INF, _INF)
    orientation: int = 2
    structure_box: Sequence[float] = (0.0, 0.0, 0.0)   # needed for reference = point with PBC


@dataclass
class DynamicNormal:
    """input/membrane_normal.rs DynamicNormal: local normals from the cloud of `heads` atoms within `radius`."""
    enabled: bool = False
    radius: float = 2.0
    cloud: Optional[np.ndarray] = None        # atom indices of group "NormalHeads"


@dataclass
class Tables:
    n_atoms: int
    molecule_types: List[MolType]
    handle_pbc: bool = True
    normal: Sequence[float] = (0.0, 0.0, 1.0)
    leaflets: Leaflets = field(default_factory=Leaflets)
    ordermap: OrderMap = field(default_factory=OrderMap)
    timewise: bool = False
    device: int = 0
    flags: int = 0          # FLAG_TRIG_ACOS_COS: acos->cos round trip like the reference
    geometry: Geometry = field(default_factory=Geometry)
    dynamic_normal: DynamicNormal = field(default_factory=DynamicNormal)

    @property
    def n_acc(self) -> int:
        return sum(m.n_slots for m in self.molecule_types)

    @property
    def n_molecules_total(self) -> int:
        return sum(m.n_molecules for m in self.molecule_types)

    @property
    def n_samples_per_frame(self) -> int:
        return sum(m.n_slots * m.n_molecules for m in self.molecule_types)

    def as_ctypes(self):
        """-> (CTables, keepalive list).  The C side copies what it needs during create()."""
        keep = []
        mts = (CMolType * max(1, len(self.molecule_types)))()
        for k, m in enumerate(self.molecule_types):
            c = mts[k]
            c.n_molecules = m.n_molecules
            b = _u32(m.bonds, (-1, m.n_molecules, 2)) if m.bonds is not None else None
            c.n_bond_types = 0 if b is None else b.shape[0]
            c.bonds = _ptr(b)
            ua = (CUaAtom * max(1, len(m.ua_atoms)))()
            for q, (kind, idx) in enumerate(m.ua_atoms):
                ia = _u32(idx, (m.n_molecules, 4))
                ua[q].kind = int(kind)
                ua[q].indices = _ptr(ia)
                keep.append(ia)
            c.n_ua_atoms = len(m.ua_atoms)
            c.ua_atoms = C.cast(ua, C.POINTER(CUaAtom))
            h = _u32(m.heads, (m.n_molecules,)) if m.heads is not None else None
            c.heads = _ptr(h)
            me = _u32(m.methyls, (m.n_molecules, -1)) if m.methyls is not None else None
            c.n_methyls = 0 if me is None else me.shape[1]
            c.methyls = _ptr(me)
            nh = _u32(m.normal_heads, (m.n_molecules,)) if m.normal_heads is not None else None
            c.normal_heads = _ptr(nh)
            keep += [b, ua, h, me, nh]
        t = CTables()
        t.n_atoms = self.n_atoms
        t.n_molecule_types = len(self.molecule_types)
        t.molecule_types = C.cast(mts, C.POINTER(CMolType))
        t.handle_pbc = 1 if self.handle_pbc else 0
        t.normal[:] = [float(x) for x in self.normal]
        lf = self.leaflets
        mem = _u32(lf.membrane) if lf.membrane is not None else None
        t.leaflets.method = lf.method
        t.leaflets.normal_dim = lf.normal_dim
        t.leaflets.frequency = lf.frequency
        t.leaflets.flip = 1 if lf.flip else 0
        t.leaflets.radius = lf.radius
        t.leaflets.n_membrane = 0 if mem is None else mem.size
        t.leaflets.membrane = _ptr(mem)
        om = self.ordermap
        t.ordermap.enabled = 1 if om.enabled else 0
        t.ordermap.plane = om.plane
        t.ordermap.span_x[:] = [float(x) for x in om.span_x]
        t.ordermap.span_y[:] = [float(x) for x in om.span_y]
        t.ordermap.bin[:] = [float(x) for x in om.bin]
        t.timewise = 1 if self.timewise else 0
        t.device = self.device
        t.flags = self.flags
        ge = self.geometry
        grp = _u32(ge.group) if ge.group is not None else None
        t.geometry.kind = ge.kind
        t.geometry.invert = 1 if ge.invert else 0
        t.geometry.reference = ge.reference
        t.geometry.point[:] = [float(x) for x in ge.point]
        t.geometry.n_group = 0 if grp is None else grp.size
        t.geometry.group = _ptr(grp)
        t.geometry.xdim[:] = [float(x) for x in ge.xdim]
        t.geometry.ydim[:] = [float(x) for x in ge.ydim]
        t.geometry.zdim[:] = [float(x) for x in ge.zdim]
        t.geometry.radius = ge.radius
        t.geometry.span[:] = [float(x) for x in ge.span]
        t.geometry.orientation = ge.orientation
        t.geometry.structure_box[:] = [float(x) for x in ge.structure_box]
        dn = self.dynamic_normal
        cloud = _u32(dn.cloud) if dn.cloud is not None else None
        t.dynamic_normal.enabled = 1 if dn.enabled else 0
        t.dynamic_normal.radius = dn.radius
        t.dynamic_normal.n_cloud = 0 if cloud is None else cloud.size
        t.dynamic_normal.cloud = _ptr(cloud)
        keep += [mts, mem, grp, cloud]
        return t, keep


# ---- the library ------------------------------------------------------------------------------
_EXPORTS = [
    "gorder_hip_create", "gorder_hip_destroy", "gorder_hip_n_accumulators", "gorder_hip_ordermap_dims",
    "gorder_hip_set_stream", "gorder_hip_submit_device", "gorder_hip_submit_host",
    "gorder_hip_prime_leaflets", "gorder_hip_set_manual_leaflets", "gorder_hip_synchronize",
    "gorder_hip_finish", "gorder_hip_timewise", "gorder_hip_leaflets", "gorder_hip_leaflet_distances",
    "gorder_hip_normals", "gorder_hip_export_maps", "gorder_hip_set_normals",
    "gorder_hip_accumulators_device", "gorder_hip_bind_accumulators", "gorder_hip_last_error_index", "gorder_hip_last_error_frame", "gorder_hip_kernel_time_names",
    "gorder_hip_last_error_message", "gorder_hip_strerror", "gorder_hip_kernel_time", "gorder_hip_kernel_time_group", "gorder_hip_plan",
    "gorder_hip_plan_tables", "gorder_hip_selftest_arithmetic", "gorder_hip_selftest_trig", "gorder_hip_selftest_wave_ops", "gorder_hip_run_trajectory",
    "gorder_hip_comm_unique_id", "gorder_hip_comm_create", "gorder_hip_comm_destroy", "gorder_hip_allreduce",
    "gorder_hip_reset", "gorder_hip_xtc_decode", "gorder_hip_release_staging", "gorder_hip_speculation_stats", "gorder_hip_local_decide_stats",
    "gorder_hip_spherical_stats", "gorder_hip_clustering_stats",
    "gorder_hip_set_collect", "gorder_hip_collected_counts", "gorder_hip_collected_leaflets", "gorder_hip_collected_normals",
    "gorder_hip_set_manual_leaflet_table", "gorder_hip_set_manual_normal_table",
    "gorder_hip_timewise_chunk_frames", "gorder_hip_timewise_rows", "gorder_hip_timewise_blocks", "gorder_hip_error_estimate",
    "gorder_hip_convergence", "gorder_hip_ordermaps",
    "gorder_hip_set_radial_shells", "gorder_hip_radial_shells", "gorder_hip_radial_thresholds",
    "gorder_hip_set_molecule_rows", "gorder_hip_molecule_rows_count", "gorder_hip_molecule_rows", "gorder_hip_molecule_rows_stats",
    "gorder_hip_set_order_histogram", "gorder_hip_order_histogram", "gorder_hip_order_histogram_route",
    "gorder_hip_set_bond_correlation", "gorder_hip_bond_correlation",
    "gorder_hip_set_neighbour_classes", "gorder_hip_neighbour_classes", "gorder_hip_neighbour_class_rows",
]

_lib = None


class GorderHipError(RuntimeError):
    def __init__(self, status: int, message: str = "", index: int = 0, frame: int = 0):
        self.status = status
        self.index = index
        self.frame = frame      # SystemTopology::frame of the first device error (gorder_hip_last_error_frame)
        super().__init__(f"gorder_hip status {status}: {message}")


def load_library() -> C.CDLL:
    """Load libgorder_hip.so (built by __graft_entry__.build / make -C gorder_amd/csrc). Fails loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GorderHipError(ERR_NO_DEVICE, f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; "
                                            "g.build()'` (there is no CPU fallback)")
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so (SONAME
    # libamdhip64.so.7, same as /opt/rocm's).  Import torch FIRST so that our DT_NEEDED entry binds to
    # the runtime torch already initialised; two runtimes in one process cannot both own the device.
    try:
        import torch  # noqa: F401
        _rt = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
        if os.path.exists(_rt):
            C.CDLL(_rt, mode=C.RTLD_GLOBAL)
    except ImportError:      # plain C/C++ hosts link against /opt/rocm directly
        pass
    lib = C.CDLL(LIB_PATH)
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    lib.gorder_hip_create.argtypes = [C.POINTER(CTables), C.POINTER(vp)]
    lib.gorder_hip_destroy.argtypes = [vp]
    lib.gorder_hip_destroy.restype = None
    lib.gorder_hip_n_accumulators.argtypes = [vp]
    lib.gorder_hip_n_accumulators.restype = u32
    lib.gorder_hip_ordermap_dims.argtypes = [vp, C.POINTER(u32), C.POINTER(u32)]
    lib.gorder_hip_ordermap_dims.restype = u32
    lib.gorder_hip_set_stream.argtypes = [vp, vp]
    lib.gorder_hip_submit_device.argtypes = [vp, vp, vp, vp, u32]
    lib.gorder_hip_submit_host.argtypes = [vp, vp, vp, vp, u32]
    lib.gorder_hip_prime_leaflets.argtypes = [vp, vp, vp, u64]
    lib.gorder_hip_set_manual_leaflets.argtypes = [vp, vp, u64]
    lib.gorder_hip_synchronize.argtypes = [vp]
    lib.gorder_hip_finish.argtypes = [vp, vp, vp, vp, vp, C.POINTER(u64)]
    lib.gorder_hip_timewise.argtypes = [vp, vp, vp, u64]
    lib.gorder_hip_leaflets.argtypes = [vp, vp, C.POINTER(u64)]
    lib.gorder_hip_leaflet_distances.argtypes = [vp, vp]
    lib.gorder_hip_normals.argtypes = [vp, vp, vp]
    lib.gorder_hip_export_maps.argtypes = [vp, vp, vp, u64]
    lib.gorder_hip_set_normals.argtypes = [vp, vp, u32]
    lib.gorder_hip_accumulators_device.argtypes = [vp, C.POINTER(vp), C.POINTER(u64)]
    lib.gorder_hip_bind_accumulators.argtypes = [vp, vp, u64]
    lib.gorder_hip_last_error_index.argtypes = [vp]
    lib.gorder_hip_last_error_index.restype = u64
    lib.gorder_hip_kernel_time_names.argtypes = [vp]
    lib.gorder_hip_kernel_time_names.restype = C.c_char_p
    lib.gorder_hip_last_error_frame.argtypes = [vp]
    lib.gorder_hip_last_error_frame.restype = u64
    lib.gorder_hip_last_error_message.argtypes = [vp]
    lib.gorder_hip_last_error_message.restype = C.c_char_p
    lib.gorder_hip_strerror.argtypes = [i32]
    lib.gorder_hip_strerror.restype = C.c_char_p
    lib.gorder_hip_kernel_time.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(u64), i32]
    lib.gorder_hip_kernel_time_group.argtypes = [vp, C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.POINTER(u64)]
    lib.gorder_hip_plan.argtypes = [vp, C.POINTER(CPlan)]
    lib.gorder_hip_speculation_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.gorder_hip_local_decide_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.gorder_hip_spherical_stats.argtypes = [vp, C.POINTER(C.c_float)]
    lib.gorder_hip_clustering_stats.argtypes = [vp, C.POINTER(C.c_float)]
    lib.gorder_hip_plan_tables.argtypes = [C.POINTER(CTables), C.POINTER(CPlan), C.POINTER(i32)]
    lib.gorder_hip_selftest_arithmetic.argtypes = [i32, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.gorder_hip_selftest_trig.argtypes = [i32, i32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.gorder_hip_selftest_wave_ops.argtypes = [i32, u32, vp, vp, vp, i32, vp, vp, vp, vp]
    lib.gorder_hip_run_trajectory.argtypes = [vp, C.POINTER(CTrajectory), C.POINTER(CTrajectoryStats)]
    lib.gorder_hip_comm_unique_id.argtypes = [vp]
    lib.gorder_hip_comm_create.argtypes = [vp, vp, i32, i32, C.POINTER(vp)]
    lib.gorder_hip_comm_destroy.argtypes = [vp]
    lib.gorder_hip_comm_destroy.restype = None
    lib.gorder_hip_allreduce.argtypes = [vp, vp]
    lib.gorder_hip_reset.argtypes = [vp]
    lib.gorder_hip_xtc_decode.argtypes = [vp, vp, u64, vp, u32, u32, vp, u32, vp, u32]
    lib.gorder_hip_release_staging.argtypes = [vp]
    lib.gorder_hip_release_staging.restype = None
    lib.gorder_hip_set_collect.argtypes = [vp, u32]
    lib.gorder_hip_collected_counts.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    lib.gorder_hip_collected_leaflets.argtypes = [vp, vp, vp, u64, C.POINTER(u64)]
    lib.gorder_hip_collected_normals.argtypes = [vp, vp, vp, u64, C.POINTER(u64)]
    lib.gorder_hip_set_manual_leaflet_table.argtypes = [vp, vp, u64, u64]
    lib.gorder_hip_set_manual_normal_table.argtypes = [vp, vp, u32, u64, u64]
    lib.gorder_hip_timewise_chunk_frames.argtypes = []
    lib.gorder_hip_timewise_chunk_frames.restype = u32
    lib.gorder_hip_timewise_rows.argtypes = [vp]
    lib.gorder_hip_timewise_rows.restype = u64
    lib.gorder_hip_timewise_blocks.argtypes = [vp, u32, u64, u64, vp, vp, C.POINTER(u64)]
    lib.gorder_hip_error_estimate.argtypes = [vp, u32, vp, vp, u32, vp, vp, vp]
    lib.gorder_hip_convergence.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, vp]
    lib.gorder_hip_ordermaps.argtypes = [vp, vp, vp, u32, u32, u32, vp, vp, u64, vp]
    lib.gorder_hip_set_radial_shells.argtypes = [vp, vp, u32]
    lib.gorder_hip_radial_shells.argtypes = [vp, vp, vp, C.POINTER(u32)]
    lib.gorder_hip_radial_thresholds.argtypes = [vp, u32, vp]
    lib.gorder_hip_set_molecule_rows.argtypes = [vp, vp, vp, u32]
    lib.gorder_hip_molecule_rows_count.argtypes = [vp, C.POINTER(u64)]
    lib.gorder_hip_molecule_rows.argtypes = [vp, vp, vp, vp, u64]
    lib.gorder_hip_molecule_rows_stats.argtypes = [vp, C.POINTER(u64), C.POINTER(u32), C.POINTER(u32)]
    lib.gorder_hip_set_order_histogram.argtypes = [vp, vp, u32]
    lib.gorder_hip_order_histogram.argtypes = [vp, vp, C.POINTER(u32)]
    lib.gorder_hip_order_histogram_route.argtypes = [vp, C.POINTER(u32), C.POINTER(u64)]
    lib.gorder_hip_set_bond_correlation.argtypes = [vp, vp, u32]
    lib.gorder_hip_bond_correlation.argtypes = [vp, vp, vp, C.POINTER(u32)]
    lib.gorder_hip_set_neighbour_classes.argtypes = [vp, vp, vp, u32, C.c_float, u32]
    lib.gorder_hip_neighbour_classes.argtypes = [vp, vp, vp, C.POINTER(u32)]
    lib.gorder_hip_neighbour_class_rows.argtypes = [vp, vp, C.POINTER(u32), C.POINTER(u32)]
    _lib = lib
    return lib


RADIAL_MAX_SHELLS = 32       # GORDER_RADIAL_MAX_SHELLS
HIST_MAX_BINS = 256          # GORDER_HIST_MAX_BINS
CORR_MAX_LAGS = 64           # GORDER_CORR_MAX_LAGS
CORR_MAX_LAG = 4096          # GORDER_CORR_MAX_LAG
NEIGHBOUR_MAX_ATOMS = 16384  # GORDER_NEIGHBOUR_MAX_ATOMS
NEIGHBOUR_MAX_CLASSES = 32   # GORDER_NEIGHBOUR_MAX_CLASSES


def radial_thresholds(radii) -> np.ndarray:
    """thr[k]: the smallest float32 whose correctly rounded square root reaches radii[k], so that `d2 < thr[k]` is exactly
    `sqrt(d2) < radii[k]` — what k_bonds_shells compares against (gorder_hip_radial_thresholds); needs no device."""
    r = np.ascontiguousarray(radii, dtype=np.float32)
    thr = np.empty(r.shape, dtype=np.float32)
    st = load_library().gorder_hip_radial_thresholds(r.ctypes.data_as(C.c_void_p), r.size, thr.ctypes.data_as(C.c_void_p))
    if st != OK:
        raise GorderHipError(st, "gorder_hip_radial_thresholds")
    return thr


def timewise_chunk_frames() -> int:
    """Rows a workgroup of the device's block-sum pass folds (gorder_hip_timewise_chunk_frames); needs no device."""
    return int(load_library().gorder_hip_timewise_chunk_frames())


def _pack_groups(groups):
    """Lists of accumulator slots -> CSR (group_begin [n + 1], slots) as the C ABI takes them."""
    begin = np.zeros(len(groups) + 1, dtype=np.uint32)
    begin[1:] = np.cumsum([len(g) for g in groups])
    flat = [int(k) for g in groups for k in g]
    slots = np.array(flat if flat else [0], dtype=np.uint32)      # (never a null pointer: the library names what is wrong)
    return begin, slots


def selftest_trig(fn: str, first_bits: int, stride: int, n: int, device: int = 0) -> np.ndarray:
    """The device's acos ('acos', 'acos_cores'), cos or sin of the floats with bit patterns first_bits + i * stride."""
    lib = load_library()
    out = np.empty(n, dtype=np.float32)
    st = lib.gorder_hip_selftest_trig(device, {"acos": 0, "acos_cores": 1, "cos": 2, "sin": 3}[fn], first_bits, stride, n, out.ctypes.data)
    if st != 0:
        raise GorderHipError(st, "gorder_hip_selftest_trig")
    return out


WAVE_OPS_ROWS = (10, 16, 9, 9)     # GORDER_WAVE_OPS_F64_ROWS, _F32_ROWS, _U32_ROWS, _FINFO_WORDS


def selftest_wave_ops(f64, f32, u32, finfo_empty: bool = False, device: int = 0):
    """What every lane of ONE workgroup of len(f64) threads holds behind each wave / block reduction of csrc/wave_ops.h
    (gorder_hip_selftest_wave_ops): (f64 [10][n], f32 [16][n], u32 [9][n], finfo [9]); the rows: include/gorder_hip.h."""
    lib = load_library()
    f64 = np.ascontiguousarray(f64, dtype=np.float64)
    f32 = np.ascontiguousarray(f32, dtype=np.float32)
    u32 = np.ascontiguousarray(u32, dtype=np.uint32)
    n = len(f64)
    if len(f32) != n or len(u32) != n:
        raise ValueError("one value of each type per thread")
    o64 = np.empty((WAVE_OPS_ROWS[0], n), dtype=np.float64)
    o32 = np.empty((WAVE_OPS_ROWS[1], n), dtype=np.float32)
    ou = np.empty((WAVE_OPS_ROWS[2], n), dtype=np.uint32)
    fi = np.empty(WAVE_OPS_ROWS[3], dtype=np.uint32)
    st = lib.gorder_hip_selftest_wave_ops(device, n, f64.ctypes.data, f32.ctypes.data, u32.ctypes.data, int(finfo_empty),
                                          o64.ctypes.data, o32.ctypes.data, ou.ctypes.data, fi.ctypes.data)
    if st != 0:
        raise GorderHipError(st, lib.gorder_hip_strerror(st).decode())
    return o64, o32, ou, fi


def selftest_arithmetic(n: int = 1 << 26, seed: int = 1, device: int = 0):
    """(division mismatches, square-root mismatches) of the kernels' Newton-core forms against the IEEE operations on
    n random operand sets inside the guarded ranges (gorder_hip_selftest_arithmetic); both must be 0."""
    lib = load_library()
    out = (C.c_uint64 * 2)()
    st = lib.gorder_hip_selftest_arithmetic(device, n, seed, out)
    if st != 0:
        raise GorderHipError(st, lib.gorder_hip_strerror(st).decode())
    return int(out[0]), int(out[1])


def plan_tables(tables: Tables) -> dict:
    """Host-only: how the library would tile these tables (no device needed)."""
    lib = load_library()
    ct, keep = tables.as_ctypes()
    plan, check = CPlan(), C.c_int(-1)
    st = lib.gorder_hip_plan_tables(C.byref(ct), C.byref(plan), C.byref(check))
    if st != OK:
        raise GorderHipError(st, lib.gorder_hip_strerror(st).decode())
    d = {name: getattr(plan, name) for name, _ in CPlan._fields_}
    d["selfcheck"] = check.value
    return d


@dataclass
class Results:
    sums: np.ndarray        # int64  [3, n_acc]   total / upper / lower
    counts: np.ndarray      # uint64 [3, n_acc]
    n_frames: int
    map_sums: Optional[np.ndarray] = None
    map_counts: Optional[np.ndarray] = None

    def order_ticks(self, min_samples: int = 1) -> np.ndarray:
        """Mean order parameter in integer ticks of 1e-6 (`OrderValue / usize`, order.rs:34-42);
        INT64_MIN marks "fewer than min_samples" (NaN in `order`)."""
        n = self.counts.astype(np.int64)
        ok = n >= max(1, min_samples)
        q = np.full(self.sums.shape, np.iinfo(np.int64).min, dtype=np.int64)
        q[ok] = (np.abs(self.sums[ok]) // n[ok]) * np.sign(self.sums[ok])
        return q

    def order(self, min_samples: int = 1) -> np.ndarray:
        """AnalysisOrder::calc_order (order.rs:101-107): truncating i64 division, then /1e6 as f32."""
        out = np.full(self.sums.shape, np.nan, dtype=np.float32)
        n = self.counts.astype(np.int64)
        ok = n >= max(1, min_samples)
        # Rust i64 `/` truncates toward zero (numpy // floors)
        q = (np.abs(self.sums[ok]) // n[ok]) * np.sign(self.sums[ok])
        out[ok] = (q.astype(np.float64) / 1e6).astype(np.float32)
        return out


class HipEngine:
    """One `SystemTopology` on one GPU (one handle per rank / stream)."""

    def __init__(self, tables: Tables):
        self.lib = load_library()
        self.tables = tables
        ct, keep = tables.as_ctypes()
        self._h = C.c_void_p()
        st = self.lib.gorder_hip_create(C.byref(ct), C.byref(self._h))
        if st != OK:
            msg = self.lib.gorder_hip_strerror(st).decode()
            if self._h:
                msg += ": " + self.lib.gorder_hip_last_error_message(self._h).decode()
                self.lib.gorder_hip_destroy(self._h)
                self._h = C.c_void_p()
            raise GorderHipError(st, msg)
        self.n_acc = self.lib.gorder_hip_n_accumulators(self._h)
        self._keep = []
        self._n_shells = 0
        self._n_mol_groups = 0

    def close(self):
        if getattr(self, "_h", None):
            self.lib.gorder_hip_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st: int):
        if st != OK:
            msg = self.lib.gorder_hip_strerror(st).decode() + ": " + \
                self.lib.gorder_hip_last_error_message(self._h).decode()
            raise GorderHipError(st, msg, self.lib.gorder_hip_last_error_index(self._h),
                                 self.lib.gorder_hip_last_error_frame(self._h))

    def set_stream(self, stream_ptr: int):
        self._check(self.lib.gorder_hip_set_stream(self._h, C.c_void_p(stream_ptr)))

    def use_torch_stream(self):
        """Launch on torch's CURRENT stream, so that torch ops (and torch.distributed collectives) issued on it are
        ordered with the handle's work.  torch's default stream is the NULL stream, which the C ABI reads as "the
        handle's own stream": make a torch.cuda.Stream current first if that ordering matters."""
        import torch
        self.set_stream(torch.cuda.current_stream().cuda_stream)

    @staticmethod
    def _frame_index(frame_index, n_frames):
        if frame_index is None:
            frame_index = np.arange(n_frames, dtype=np.uint64)
        fi = np.ascontiguousarray(frame_index, dtype=np.uint64)
        assert fi.shape == (n_frames,)
        return fi

    def submit_device(self, xyz, box, frame_index=None):
        """xyz: torch float32 CUDA tensor [F, N, 3]; box: [F, 3, 3] (or None when handle_pbc=False)."""
        assert xyz.is_cuda and xyz.is_contiguous() and xyz.dtype.is_floating_point and xyz.element_size() == 4
        n_frames = xyz.shape[0]
        assert xyz.shape[1] == self.tables.n_atoms and xyz.shape[2] == 3
        fi = self._frame_index(frame_index, n_frames)
        bp = None
        if box is not None:
            assert box.is_cuda and box.is_contiguous() and box.numel() == 9 * n_frames
            bp = C.c_void_p(box.data_ptr())
        self._check(self.lib.gorder_hip_submit_device(self._h, C.c_void_p(xyz.data_ptr()), bp,
                                                      fi.ctypes.data_as(C.c_void_p), n_frames))

    def submit_host(self, xyz: np.ndarray, box: Optional[np.ndarray], frame_index=None):
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        n_frames = xyz.shape[0]
        assert xyz.shape[1:] == (self.tables.n_atoms, 3)
        fi = self._frame_index(frame_index, n_frames)
        bp = None
        if box is not None:
            box = np.ascontiguousarray(box, dtype=np.float32).reshape(n_frames, 9)
            bp = box.ctypes.data_as(C.c_void_p)
        self._check(self.lib.gorder_hip_submit_host(self._h, xyz.ctypes.data_as(C.c_void_p), bp,
                                                    fi.ctypes.data_as(C.c_void_p), n_frames))

    def run_trajectory(self, paths, group=None, begin: float = 0.0, end: float = -1.0, step: int = 1, threads: int = 0,
                       batch_frames: int = 0, first_frame_index: int = 0, device_decode: bool = False,
                       shard=None) -> dict:
        """The reference's `read_trajectory` (common.rs:239-342) as one library call: read (and concatenate) the
        files, apply the time window / step, decode on `threads` host threads and analyse batch by batch with copies
        and kernels overlapped (gorder_hip_run_trajectory).  `device_decode`: the host threads only copy the compressed
        XTC blocks, the device unpacks them (k_xtc_scan + k_xtc_chunks); of TRR files the positions of the analysed atoms
        travel as they are in the file and k_trr_unpack makes the floats.  A GRO file in the run: host decoder.  `shard` = (i, n): analyse only the i-th of n
        contiguous shares of the selected frames (one rank of a multi-GPU run).  -> the pipeline's statistics."""
        arr = (C.c_char_p * len(paths))(*[p.encode() for p in paths])
        grp = None if group is None else np.ascontiguousarray(group, dtype=np.uint32)
        t = CTrajectory()
        t.paths = C.cast(arr, C.POINTER(C.c_char_p))
        t.n_paths = len(paths)
        t.group = _ptr(grp)
        t.n_group = 0 if grp is None else grp.size
        t.begin_ps, t.end_ps, t.step = begin, end, step
        t.n_threads, t.batch_frames, t.first_frame_index = threads, batch_frames, first_frame_index
        t.device_decode = 1 if device_decode else 0
        if shard is not None:          # (index, count): this rank's contiguous share of the selected frames
            t.shard_index, t.shard_count = shard
        stats = CTrajectoryStats()
        self._check(self.lib.gorder_hip_run_trajectory(self._h, C.byref(t), C.byref(stats)))
        return {name: getattr(stats, name) for name, _ in CTrajectoryStats._fields_}

    def xtc_decode(self, d_blob: int, blob_bytes: int, d_frames: int, n_frames: int, n_atoms_file: int, d_slot_of: int,
                   n_stop: int, d_xyz: int, n_atoms_out: int):
        """Decompress packed XTC frames — and unpack packed TRR frames, also in one table — on the device
        (gorder_hip_xtc_decode); all pointers are device addresses (d_slot_of may be 0).  The kernels are asynchronous on
        the handle's stream; the call first reads the table's `kind` words back in that stream's order."""
        self._check(self.lib.gorder_hip_xtc_decode(self._h, d_blob, blob_bytes, d_frames, n_frames, n_atoms_file,
                                                   d_slot_of or None, n_stop, d_xyz, n_atoms_out))

    def release_staging(self):
        """Give back the staging buffers run_trajectory keeps between calls (gorder_hip_release_staging)."""
        self.lib.gorder_hip_release_staging(self._h)

    def reset(self):
        """A fresh SystemTopology on the same tables (gorder_hip_reset)."""
        self._check(self.lib.gorder_hip_reset(self._h))

    @staticmethod
    def comm_unique_id() -> bytes:
        """Rank 0: the 128-byte RCCL id the other ranks need for comm_create (ship it over any channel)."""
        lib = load_library()
        buf = (C.c_uint8 * 128)()
        st = lib.gorder_hip_comm_unique_id(buf)
        if st != OK:
            raise GorderHipError(st, "ncclGetUniqueId failed (is RCCL loadable?)")
        return bytes(buf)

    def comm_create(self, unique_id: bytes, n_ranks: int, rank: int):
        """An RCCL communicator (ncclComm_t) on this handle's device -> opaque pointer for allreduce()."""
        assert len(unique_id) == 128
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        comm = C.c_void_p()
        self._check(self.lib.gorder_hip_comm_create(self._h, buf, n_ranks, rank, C.byref(comm)))
        return comm

    def comm_destroy(self, comm):
        self.lib.gorder_hip_comm_destroy(comm)

    def allreduce(self, comm):
        """SystemTopology::reduce across the ranks of `comm`: one group of RCCL all-reduces issued by the library."""
        self._check(self.lib.gorder_hip_allreduce(self._h, comm))

    def prime_leaflets_device(self, xyz, box, frame_index: int):
        bp = C.c_void_p(box.data_ptr()) if box is not None else None
        self._check(self.lib.gorder_hip_prime_leaflets(self._h, C.c_void_p(xyz.data_ptr()), bp, frame_index))

    def set_manual_leaflets(self, flags: np.ndarray, frame_index: int = 0):
        flags = np.ascontiguousarray(flags, dtype=np.uint8)
        assert flags.size == self.tables.n_molecules_total
        self._check(self.lib.gorder_hip_set_manual_leaflets(self._h, flags.ctypes.data_as(C.c_void_p), frame_index))

    def set_manual_leaflet_table(self, flags, first_row: int = 0):
        """Manual leaflets of the whole trajectory (gorder_hip_set_manual_leaflet_table): flags [rows, n_molecules_total],
        Upper = 0 / Lower = 1, row r = assignment index first_row + r (frame // frequency; 0 for frequency 0) — what
        collected_leaflets() or manual.read_leaflets_file gives.  Copied to the device; zero rows (or None) remove the table."""
        n_mol = self.tables.n_molecules_total
        flags = np.zeros((0, n_mol), dtype=np.uint8) if flags is None else np.ascontiguousarray(flags, dtype=np.uint8)
        assert flags.ndim == 2 and flags.shape[1] == n_mol
        self._check(self.lib.gorder_hip_set_manual_leaflet_table(self._h, flags.ctypes.data_as(C.c_void_p) if len(flags) else None,
                                                                 first_row, len(flags)))

    def set_manual_normal_table(self, normals, step: int = 1, first_row: int = 0):
        """Manual membrane normals of the whole trajectory (gorder_hip_set_manual_normal_table): normals
        [rows, n_molecules_total, 3], row r = frame (first_row + r) * step — what collected_normals() or
        manual.read_normals_file gives.  Copied to the device; zero rows (or None) remove the table."""
        n_mol = self.tables.n_molecules_total
        n = np.zeros((0, n_mol, 3), dtype=np.float32) if normals is None else np.ascontiguousarray(normals, dtype=np.float32)
        assert n.ndim == 3 and n.shape[1:] == (n_mol, 3)
        self._check(self.lib.gorder_hip_set_manual_normal_table(self._h, n.ctypes.data_as(C.c_void_p) if len(n) else None,
                                                                step, first_row, len(n)))

    def synchronize(self):
        self._check(self.lib.gorder_hip_synchronize(self._h))

    def ordermap_dims(self):
        """(nx, ny) tiles of every ordermap; (0, 0) when ordermaps are off."""
        nx, ny = C.c_uint32(), C.c_uint32()
        nt = self.lib.gorder_hip_ordermap_dims(self._h, C.byref(nx), C.byref(ny))
        return (int(nx.value), int(ny.value)) if nt else (0, 0)

    def finish(self) -> Results:
        n = self.n_acc
        sums = np.zeros((3, n), dtype=np.int64)
        counts = np.zeros((3, n), dtype=np.uint64)
        nx, ny = C.c_uint32(), C.c_uint32()
        nt = self.lib.gorder_hip_ordermap_dims(self._h, C.byref(nx), C.byref(ny))
        ms = mc = None
        msp = mcp = None
        if nt:
            ms = np.zeros((3, n, nx.value, ny.value), dtype=np.int64)
            mc = np.zeros((3, n, nx.value, ny.value), dtype=np.uint64)
            msp, mcp = ms.ctypes.data_as(C.c_void_p), mc.ctypes.data_as(C.c_void_p)
        nf = C.c_uint64()
        self._check(self.lib.gorder_hip_finish(self._h, sums.ctypes.data_as(C.c_void_p),
                                               counts.ctypes.data_as(C.c_void_p), msp, mcp, C.byref(nf)))
        return Results(sums, counts, int(nf.value), ms, mc)

    def timewise(self, n_frames: int):
        n = self.n_acc
        s = np.zeros((n_frames, 3, n), dtype=np.int64)
        c = np.zeros((n_frames, 3, n), dtype=np.uint64)
        self._check(self.lib.gorder_hip_timewise(self._h, s.ctypes.data_as(C.c_void_p),
                                                 c.ctypes.data_as(C.c_void_p), n_frames))
        return s, c

    def timewise_rows(self) -> int:
        """Per-frame rows the handle holds: the frames analysed since it was made or reset (0 with timewise off)."""
        return int(self.lib.gorder_hip_timewise_rows(self._h))

    def timewise_blocks(self, n_blocks: int, total_frames: Optional[int] = None, first_position: int = 0):
        """Block sums of the handle's rows, made on the device (gorder_hip_timewise_blocks) -> (sums int64, counts uint64
        [n_blocks, 3, n_acc], block_size).  The block grid is that of an analysis of `total_frames` frames (default: this
        handle's rows) in which the handle's first row sits at `first_position`; the outputs of the shards of one analysis
        add up element by element to the block sums of the whole run."""
        if total_frames is None:
            total_frames = self.timewise_rows()
        s = np.zeros((n_blocks, 3, self.n_acc), dtype=np.int64)
        c = np.zeros((n_blocks, 3, self.n_acc), dtype=np.uint64)
        bs = C.c_uint64()
        self._check(self.lib.gorder_hip_timewise_blocks(self._h, n_blocks, total_frames, first_position, s.ctypes.data_as(C.c_void_p),
                                                        c.ctypes.data_as(C.c_void_p), C.byref(bs)))
        return s, c, int(bs.value)

    def error_estimate(self, groups, n_blocks: int = 5, blocks=None) -> np.ndarray:
        """estimate_error of every group (a list of accumulator slots whose rows are added) and leaflet, on the device
        (gorder_hip_error_estimate) -> float32 [n_groups, 3], bit for bit structure.estimate_error on the rows.
        blocks = (sums, counts) [n_blocks, 3, n_acc]: the merged timewise_blocks() of the shards instead of this handle's rows."""
        begin, slots = _pack_groups(groups)
        out = np.zeros((len(groups), 3), dtype=np.float32)
        bs = bc = None
        if blocks is not None:
            bs = np.ascontiguousarray(blocks[0], dtype=np.int64)
            bc = np.ascontiguousarray(blocks[1], dtype=np.uint64)
            assert bs.shape == bc.shape == (n_blocks, 3, self.n_acc)
        self._check(self.lib.gorder_hip_error_estimate(self._h, n_blocks, begin.ctypes.data_as(C.c_void_p), slots.ctypes.data_as(C.c_void_p),
                                                       len(groups), None if bs is None else bs.ctypes.data_as(C.c_void_p),
                                                       None if bc is None else bc.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
        return out

    def convergence(self, groups, carry=None):
        """Running averages of every group and leaflet over the handle's rows, on the device (gorder_hip_convergence) ->
        (prefix float32 [rows, 3, n_groups]: NaN while nothing was sampled, no sign flip; end = (sums int64, counts uint64)
        [3, n_groups] behind the last row).  carry: the `end` of the shard before this one."""
        begin, slots = _pack_groups(groups)
        n = len(groups)
        prefix = np.zeros((self.timewise_rows(), 3, n), dtype=np.float32)
        es, ec = np.zeros((3, n), dtype=np.int64), np.zeros((3, n), dtype=np.uint64)
        cs = cc = None
        if carry is not None:
            cs = np.ascontiguousarray(carry[0], dtype=np.int64)
            cc = np.ascontiguousarray(carry[1], dtype=np.uint64)
            assert cs.shape == cc.shape == (3, n)
        self._check(self.lib.gorder_hip_convergence(self._h, begin.ctypes.data_as(C.c_void_p), slots.ctypes.data_as(C.c_void_p), n,
                                                    None if cs is None else cs.ctypes.data_as(C.c_void_p),
                                                    None if cc is None else cc.ctypes.data_as(C.c_void_p),
                                                    prefix.ctypes.data_as(C.c_void_p), es.ctypes.data_as(C.c_void_p),
                                                    ec.ctypes.data_as(C.c_void_p)))
        return prefix, (es, ec)

    def ordermaps(self, groups, min_samples: int = 1, negate: bool = True, device_maps=None) -> np.ndarray:
        """The finished ordermap of every group (a list of accumulator slots whose tiles are added) and plane, made on the
        device (gorder_hip_ordermaps) -> float32 [n_groups, 3, nx, ny] (total, upper, lower; NaN below min_samples, and in
        the upper and lower planes without leaflets), bit for bit structure.ordermap_values on finish()'s maps.
        negate: True for all-atom and united-atom analyses (-S), False for coarse-grained.
        device_maps = (sums, counts): two torch.int64 CUDA tensors in export_maps' layout — the maps of several ranks added
        up — instead of this handle's own maps."""
        begin, slots = _pack_groups(groups)
        nx, ny = self.ordermap_dims()
        out = np.zeros((len(groups), 3, nx, ny), dtype=np.float32)
        buf = out if out.size else np.zeros(1, dtype=np.float32)      # (never a null pointer: the library names what is wrong)
        ds = dc = None
        n_u64 = 0
        if device_maps is not None:
            import torch
            ds, dc = device_maps
            for t in (ds, dc):
                assert t.is_cuda and t.is_contiguous() and t.element_size() == 8
            assert ds.numel() == dc.numel()
            n_u64 = ds.numel()
            torch.cuda.synchronize(ds.device)          # the tensors are torch's work: complete before the handle's stream reads them
        self._check(self.lib.gorder_hip_ordermaps(self._h, begin.ctypes.data_as(C.c_void_p), slots.ctypes.data_as(C.c_void_p), len(groups),
                                                  int(min_samples), 1 if negate else 0,
                                                  None if ds is None else C.c_void_p(ds.data_ptr()),
                                                  None if dc is None else C.c_void_p(dc.data_ptr()), n_u64,
                                                  buf.ctypes.data_as(C.c_void_p)))
        return out

    def leaflets(self):
        flags = np.zeros(self.tables.n_molecules_total, dtype=np.uint8)
        fr = C.c_uint64()
        self._check(self.lib.gorder_hip_leaflets(self._h, flags.ctypes.data_as(C.c_void_p), C.byref(fr)))
        return flags, int(fr.value)

    def set_collect(self, what: int):
        """Keep every assignment frame's leaflet flags (COLLECT_LEAFLETS) and / or every analysed frame's dynamic membrane
        normals (COLLECT_NORMALS) of the frames submitted from now on (gorder_hip_set_collect): before the first submit
        or right after reset()."""
        self._check(self.lib.gorder_hip_set_collect(self._h, what))

    def set_radial_shells(self, radii):
        """Ascending radii (nm) around the reference of the tables' cylinder or sphere, the last one geometry.radius: from
        now on the handle also keeps sums and counts per shell radii[k - 1] <= d < radii[k] (gorder_hip_set_radial_shells).
        Before the first submit or right after reset(); an empty list switches the shells off."""
        r = np.ascontiguousarray([] if radii is None else radii, dtype=np.float32).reshape(-1)
        self._check(self.lib.gorder_hip_set_radial_shells(self._h, r.ctypes.data_as(C.c_void_p) if r.size else None, r.size))
        self._n_shells = int(r.size)

    def radial_shells(self) -> List[Results]:
        """One Results per shell (sums, counts [3, n_acc] as finish() gives them, n_frames the frames analysed so far): raw
        integers, the shells of several shards add up element by element (gorder_hip_radial_shells).  Waits like finish()."""
        n = C.c_uint32()
        k = self._n_shells
        sums = np.zeros((max(k, 1), 3, self.n_acc), dtype=np.int64)
        counts = np.zeros((max(k, 1), 3, self.n_acc), dtype=np.uint64)
        self._check(self.lib.gorder_hip_radial_shells(self._h, sums.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p), C.byref(n)))
        assert n.value == k
        nf = C.c_uint64()
        self._check(self.lib.gorder_hip_finish(self._h, None, None, None, None, C.byref(nf)))
        return [Results(sums[q], counts[q], int(nf.value)) for q in range(k)]

    def set_molecule_rows(self, groups):
        """Keep, from now on, every molecule's own tick sum and sample count per analysed frame and group — a group is a list
        of accumulator slots, the groups are disjoint (gorder_hip_set_molecule_rows; structure.molecule_groups makes one per
        molecule type).  Before the first submit or right after reset(); an empty list switches the rows off."""
        groups = [] if groups is None else list(groups)
        begin, slots = _pack_groups(groups)
        self._check(self.lib.gorder_hip_set_molecule_rows(self._h, begin.ctypes.data_as(C.c_void_p), slots.ctypes.data_as(C.c_void_p),
                                                          len(groups)))
        self._n_mol_groups = len(groups)

    def set_order_histogram(self, edges):
        """Ascending integer tick edges (structure.order_edges, structure.tilt_edges): from now on the handle also counts the
        samples per bin edges[k] <= tick < edges[k + 1], accumulator slot and leaflet (gorder_hip_set_order_histogram).  Before
        the first submit or right after reset(); an empty list switches the histogram off."""
        e = np.asarray([] if edges is None else edges).reshape(-1)
        if e.size and (not np.issubdtype(e.dtype, np.integer) or e.min() < -2**31 or e.max() >= 2**31):
            raise ValueError("the edges are int32 ticks")
        e = np.ascontiguousarray(e, dtype=np.int32)
        self._check(self.lib.gorder_hip_set_order_histogram(self._h, e.ctypes.data_as(C.c_void_p) if e.size else None, e.size))

    def order_histogram_route(self) -> dict:
        """Which route the histogram takes (gorder_hip_order_histogram_route): "direct" — per-sample global atomics, because the
        LDS table of the widest tile does not fit or GORDER_HIP_DIST_DIRECT is set — and the table's size in bytes."""
        d, b = C.c_uint32(), C.c_uint64()
        self._check(self.lib.gorder_hip_order_histogram_route(self._h, C.byref(d), C.byref(b)))
        return {"direct": bool(d.value), "table_bytes": int(b.value)}

    def order_histogram(self) -> np.ndarray:
        """Sample counts uint64 [n_bins, 3, n_acc] (total, upper, lower) of the frames analysed so far: raw integers, the
        arrays of several shards add up (gorder_hip_order_histogram).  Waits like finish(); [0, 3, n_acc] with the
        histogram off."""
        n = C.c_uint32()
        self._check(self.lib.gorder_hip_order_histogram(self._h, None, C.byref(n)))
        counts = np.zeros((n.value, 3, self.n_acc), dtype=np.uint64)
        if n.value:
            self._check(self.lib.gorder_hip_order_histogram(self._h, counts.ctypes.data_as(C.c_void_p), C.byref(n)))
        return counts

    def set_bond_correlation(self, lags):
        """Strictly ascending lags in analysed frames (structure.correlation_lags; 1 to CORR_MAX_LAGS values, none above
        CORR_MAX_LAG, 0 allowed): from now on the handle also books, per lag, accumulator slot and leaflet, the P2 tick of every
        bond vector against its own vector `lag` analysed frames earlier (gorder_hip_set_bond_correlation).  Before the first
        submit or right after reset(); an empty list switches the correlation off."""
        l = np.asarray([] if lags is None else lags).reshape(-1)
        if l.size and (not np.issubdtype(l.dtype, np.integer) or l.min() < 0 or l.max() >= 2**32):
            raise ValueError("the lags are non-negative integers")
        l = np.ascontiguousarray(l, dtype=np.uint32)
        self._check(self.lib.gorder_hip_set_bond_correlation(self._h, l.ctypes.data_as(C.c_void_p) if l.size else None, l.size))

    def bond_correlation(self):
        """(sums int64 [n_lags, 3, n_acc], counts uint64 [n_lags, 3, n_acc]) of the frames analysed so far, the planes total,
        upper, lower: raw integers, C = sums / counts / 1e6 (structure.correlation_values), the arrays of several shards add
        up (gorder_hip_bond_correlation).  Waits like finish(); [0, 3, n_acc] with the correlation off."""
        n = C.c_uint32()
        self._check(self.lib.gorder_hip_bond_correlation(self._h, None, None, C.byref(n)))
        sums = np.zeros((n.value, 3, self.n_acc), dtype=np.int64)
        counts = np.zeros((n.value, 3, self.n_acc), dtype=np.uint64)
        if n.value:
            self._check(self.lib.gorder_hip_bond_correlation(self._h, sums.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p),
                                                             C.byref(n)))
        return sums, counts

    def set_neighbour_classes(self, centres, neighbours, radius, n_classes):
        """One centre atom per molecule (structure.neighbour_centres: the heads), strictly ascending neighbour atoms (1 to
        NEIGHBOUR_MAX_ATOMS), a radius in nm and 2 to NEIGHBOUR_MAX_CLASSES classes: from now on the handle also books every
        bond sample on the class min(neighbour atoms within the radius of its molecule's centre, n_classes - 1) of its frame
        (gorder_hip_set_neighbour_classes).  Before the first submit or right after reset(); an empty neighbour list switches
        the feature off."""
        def atoms(a):
            a = np.asarray([] if a is None else a).reshape(-1)
            if a.size and (not np.issubdtype(a.dtype, np.integer) or a.min() < 0 or a.max() >= 2**32):
                raise ValueError("atom indices are non-negative integers")
            return np.ascontiguousarray(a, dtype=np.uint32)
        c, q = atoms(centres), atoms(neighbours)
        if q.size and c.size != self.tables.n_molecules_total:
            raise ValueError("one centre per molecule")
        self._check(self.lib.gorder_hip_set_neighbour_classes(self._h, c.ctypes.data_as(C.c_void_p) if c.size else None,
                                                              q.ctypes.data_as(C.c_void_p) if q.size else None, q.size,
                                                              float(radius), int(n_classes)))

    def neighbour_classes(self) -> List[Results]:
        """One Results per class (sums, counts [3, n_acc] as finish() gives them, n_frames the frames analysed so far): raw
        integers, the classes of several shards add up element by element (gorder_hip_neighbour_classes).  Waits like
        finish(); an empty list with the feature off."""
        n = C.c_uint32()
        self._check(self.lib.gorder_hip_neighbour_classes(self._h, None, None, C.byref(n)))
        k = int(n.value)
        sums = np.zeros((max(k, 1), 3, self.n_acc), dtype=np.int64)
        counts = np.zeros((max(k, 1), 3, self.n_acc), dtype=np.uint64)
        if k:
            self._check(self.lib.gorder_hip_neighbour_classes(self._h, sums.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p), C.byref(n)))
        nf = C.c_uint64()
        self._check(self.lib.gorder_hip_finish(self._h, None, None, None, None, C.byref(nf)))
        return [Results(sums[q], counts[q], int(nf.value)) for q in range(k)]

    def neighbour_class_rows(self) -> np.ndarray:
        """The class bytes uint8 [frames, n_molecules_total] of the last submitted batch (gorder_hip_neighbour_class_rows): a
        diagnostic.  Waits like finish(); [0, 0] with the feature off or nothing submitted."""
        nf, nm = C.c_uint32(), C.c_uint32()
        self._check(self.lib.gorder_hip_neighbour_class_rows(self._h, None, C.byref(nf), C.byref(nm)))
        rows = np.zeros((nf.value, nm.value), dtype=np.uint8)
        if rows.size:
            self._check(self.lib.gorder_hip_neighbour_class_rows(self._h, rows.ctypes.data_as(C.c_void_p), C.byref(nf), C.byref(nm)))
        return rows

    def molecule_rows_count(self) -> int:
        """Per-molecule rows kept so far (one per analysed frame); does not wait."""
        n = C.c_uint64()
        self._check(self.lib.gorder_hip_molecule_rows_count(self._h, C.byref(n)))
        return int(n.value)

    def molecule_rows_stats(self) -> dict:
        """Facts of the lane order built by set_molecule_rows (gorder_hip_molecule_rows_stats): n_runs = global atomics per
        frame, max_runs_per_tile, max_tiles_per_word = tiles that add into one (group, molecule) word."""
        a, b, c = C.c_uint64(), C.c_uint32(), C.c_uint32()
        self._check(self.lib.gorder_hip_molecule_rows_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"n_runs": int(a.value), "max_runs_per_tile": int(b.value), "max_tiles_per_word": int(c.value)}

    def molecule_rows(self):
        """Every analysed frame since set_molecule_rows / reset -> (sums int32 [rows, n_groups, n_molecules_total]: tick sums
        of each molecule's samples in each group, counts uint32 likewise, frames uint64 [rows]: the frames' global indices).
        Waits like finish().  structure.molecule_order turns them into order parameters."""
        rows = self.molecule_rows_count()
        shape = (rows, self._n_mol_groups, self.tables.n_molecules_total)
        sums, counts = np.zeros(shape, dtype=np.int32), np.zeros(shape, dtype=np.uint32)
        frames = np.zeros(rows, dtype=np.uint64)
        self._check(self.lib.gorder_hip_molecule_rows(self._h, sums.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p),
                                                      frames.ctypes.data_as(C.c_void_p), rows))
        rows_now = self.molecule_rows_count()      # (a device error that surfaced while waiting drops the failed batch's rows)
        return sums[:rows_now], counts[:rows_now], frames[:rows_now]

    def collected_counts(self):
        """(leaflet rows, normal rows) collected so far; does not wait."""
        a, b = C.c_uint64(), C.c_uint64()
        self._check(self.lib.gorder_hip_collected_counts(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def collected_leaflets(self):
        """Every assignment frame since set_collect / reset -> (flags [rows, n_molecules_total] u8, Upper = 0 / Lower = 1,
        frames [rows] u64: the frames' global indices)."""
        rows = self.collected_counts()[0]
        flags = np.zeros((rows, self.tables.n_molecules_total), dtype=np.uint8)
        frames = np.zeros(rows, dtype=np.uint64)
        n = C.c_uint64()
        self._check(self.lib.gorder_hip_collected_leaflets(self._h, flags.ctypes.data_as(C.c_void_p),
                                                           frames.ctypes.data_as(C.c_void_p), rows, C.byref(n)))
        assert n.value == rows
        return flags, frames

    def collected_normals(self):
        """Every analysed frame since set_collect / reset -> (normals [rows, n_molecules_total, 3] f32, NaN where the
        reference never computed the molecule's normal in that frame, frames [rows] u64)."""
        rows = self.collected_counts()[1]
        normals = np.zeros((rows, self.tables.n_molecules_total, 3), dtype=np.float32)
        frames = np.zeros(rows, dtype=np.uint64)
        n = C.c_uint64()
        self._check(self.lib.gorder_hip_collected_normals(self._h, normals.ctypes.data_as(C.c_void_p),
                                                          frames.ctypes.data_as(C.c_void_p), rows, C.byref(n)))
        assert n.value == rows
        return normals, frames

    def leaflet_distances(self) -> np.ndarray:
        d = np.zeros(self.tables.n_molecules_total, dtype=np.float32)
        self._check(self.lib.gorder_hip_leaflet_distances(self._h, d.ctypes.data_as(C.c_void_p)))
        return d

    def set_normals(self, normals: np.ndarray):
        """Manual membrane normals [n_frames, n_molecules_total, 3] for the NEXT submit call."""
        n = np.ascontiguousarray(normals, dtype=np.float32)
        assert n.ndim == 3 and n.shape[1:] == (self.tables.n_molecules_total, 3)
        self._check(self.lib.gorder_hip_set_normals(self._h, n.ctypes.data_as(C.c_void_p), n.shape[0]))

    def normals(self):
        """Dynamic membrane normals of the last submitted frame -> (normals [n_mol, 3] f32, n_points [n_mol])."""
        n = np.zeros((self.tables.n_molecules_total, 3), dtype=np.float32)
        k = np.zeros(self.tables.n_molecules_total, dtype=np.uint32)
        self._check(self.lib.gorder_hip_normals(self._h, n.ctypes.data_as(C.c_void_p), k.ctypes.data_as(C.c_void_p)))
        return n, k

    def accumulator_words(self) -> int:
        p, n = C.c_void_p(), C.c_uint64()
        self._check(self.lib.gorder_hip_accumulators_device(self._h, C.byref(p), C.byref(n)))
        return int(n.value)

    def flush(self):
        """Make the packed accumulator block complete (stream-ordered) — call before a collective on it."""
        self.accumulator_words()

    def bind_accumulators(self, tensor):
        """Accumulate into a caller-owned torch.int64 CUDA tensor (so that torch.distributed can
        all-reduce it over RCCL)."""
        assert tensor.is_cuda and tensor.is_contiguous() and tensor.element_size() == 8
        self._keep.append(tensor)
        self._check(self.lib.gorder_hip_bind_accumulators(self._h, C.c_void_p(tensor.data_ptr()), tensor.numel()))

    def export_maps(self, sums, counts):
        """Copy the ordermaps (i64 sums, u64 counts, [3][n_acc][nx*ny]) into two caller-owned torch.int64 CUDA
        tensors so that torch.distributed can all-reduce them like the accumulator block."""
        for t in (sums, counts):
            assert t.is_cuda and t.is_contiguous() and t.element_size() == 8
        assert sums.numel() == counts.numel()
        self._check(self.lib.gorder_hip_export_maps(self._h, C.c_void_p(sums.data_ptr()), C.c_void_p(counts.data_ptr()),
                                                     sums.numel()))

    def kernel_time(self, reset: bool = False):
        ms, n = C.c_double(), C.c_uint64()
        self._check(self.lib.gorder_hip_kernel_time(self._h, C.byref(ms), C.byref(n), 1 if reset else 0))
        return ms.value, int(n.value)

    def kernel_names(self) -> str:
        """The kernel groups gorder_hip_kernel_time has measured since the last reset, joined by ' + '."""
        return self.lib.gorder_hip_kernel_time_names(self._h).decode()

    def kernel_groups(self):
        """[(name, ms, segments)] per kernel group of the timed submits since the last reset (the times add up to
        kernel_time()'s ms).  Call before kernel_time(reset=True)."""
        out, k = [], 0
        while True:
            name, ms, n = C.c_char_p(), C.c_double(), C.c_uint64()
            if self.lib.gorder_hip_kernel_time_group(self._h, k, C.byref(name), C.byref(ms), C.byref(n)) != 0:
                return out
            out.append((name.value.decode(), ms.value, int(n.value)))
            k += 1

    def speculation_stats(self) -> dict:
        """One-read global leaflets (gorder_hip_speculation_stats): batches run that way, pairs moved, frames left to the
        exact kernel, and whether the handle still speculates."""
        out = (C.c_uint64 * 4)()
        self._check(self.lib.gorder_hip_speculation_stats(self._h, out))
        return {"batches": int(out[0]), "moved": int(out[1]), "exact_frames": int(out[2]), "enabled": bool(out[3])}

    def local_decide_stats(self) -> dict:
        """Local leaflets (gorder_hip_local_decide_stats): submits that ran the bound kernel, submits that paused it, and the
        last report read back (frames left open, frames seen)."""
        out = (C.c_uint64 * 4)()
        self._check(self.lib.gorder_hip_local_decide_stats(self._h, out))
        return {"submits": int(out[0]), "paused": int(out[1]), "open_frames": int(out[2]), "frames": int(out[3])}

    def spherical_stats(self) -> dict:
        """Spherical clustering (gorder_hip_spherical_stats), most recent assignment frame: centre of the head group, the
        fitted two-component mixture, final average log-likelihood, EM iterations, group atoms labelled outer."""
        out = (C.c_float * 12)()
        self._check(self.lib.gorder_hip_spherical_stats(self._h, out))
        v = np.array(out[:], dtype=np.float32)
        return {"centre": v[0:3].copy(), "weight_a": v[3], "mean_a": v[4], "var_a": v[5], "mean_b": v[6], "var_b": v[7],
                "avg_log_likelihood": v[8], "iterations": int(v[9]), "n_outer": int(v[10])}

    def clustering_stats(self) -> dict:
        """Spectral clustering (gorder_hip_clustering_stats), most recent assignment frame: eigenvalues 2-4 of the normalised
        Laplacian, Lanczos steps, 2-means rounds, populations of the two clusters before and after orientation, the overlaps
        with the previous assignment frame's leaflets (NaN for frame 0)."""
        out = (C.c_float * 12)()
        self._check(self.lib.gorder_hip_clustering_stats(self._h, out))
        v = np.array(out[:], dtype=np.float32)
        return {"eigenvalues": v[0:3].copy(), "steps": int(v[3]), "rounds": int(v[4]), "n_cluster": (int(v[5]), int(v[6])),
                "n_upper": int(v[7]), "n_lower": int(v[8]), "o_up": v[9], "o_lo": v[10]}

    def plan(self) -> dict:
        p = CPlan()
        self._check(self.lib.gorder_hip_plan(self._h, C.byref(p)))
        return {name: getattr(p, name) for name, _ in CPlan._fields_}
