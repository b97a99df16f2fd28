"""Handles without manual tables whose kernel groups tests/test_replay_gpu.py pins: what each queues for one batch, as
gorder_hip_kernel_time_names reports it.  Run as a script it prints the names as JSON; with GORDER_HIP_LIB pointing at a
library built from the commit before the tables existed, those are the strings the test pins."""
import json

import numpy as np

from gorder_amd import HipEngine, synthetic
from gorder_amd.abi import LEAFLETS_GLOBAL, LEAFLETS_MANUAL, DynamicNormal


def _cg_dynamic():
    system = synthetic.cg_membrane(64)
    mt = system.tables.molecule_types[0]
    mt.normal_heads = (np.arange(64) * 12 + 1).astype(np.uint32)
    system.tables.dynamic_normal = DynamicNormal(enabled=True, radius=2.0, cloud=mt.normal_heads)
    return system


CASES = {
    "aa70 manual leaflets, one row": (lambda: synthetic.aa_membrane(70, leaflets=LEAFLETS_MANUAL), "leaflets"),
    "cg90 global leaflets, set_normals": (lambda: synthetic.cg_membrane(90, leaflets=LEAFLETS_GLOBAL, n_types=2), "normals"),
    "ua30 global leaflets, set_normals": (lambda: synthetic.ua_membrane(30, leaflets=LEAFLETS_GLOBAL), "normals"),
    "cg40 plain": (lambda: synthetic.cg_membrane(40), None),
    "cg64 dynamic normals": (_cg_dynamic, None),
}


def names_of(case: str) -> str:
    make, manual = CASES[case]
    system = make()
    n, n_mol = 5, system.tables.n_molecules_total
    eng = HipEngine(system.tables)
    eng.kernel_time(reset=True)
    if manual == "leaflets":
        eng.set_manual_leaflets((np.arange(n_mol) % 2).astype(np.uint8), 0)
    elif manual == "normals":
        z = np.zeros((n, n_mol, 3), dtype=np.float32)
        z[:, :, 2] = 1.0
        eng.set_normals(z)
    eng.submit_host(system.frames(n, seed=2), system.box9(n), np.arange(n))
    eng.finish()
    eng.kernel_time()
    return eng.kernel_names()


if __name__ == "__main__":
    print(json.dumps({case: names_of(case) for case in CASES}, indent=1))
