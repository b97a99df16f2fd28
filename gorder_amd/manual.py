"""Readers for the reference's two manual-input files: the leaflet assignment file (`!FromFile`, leaflets.rs:815-858) and
the membrane normals file (normal.rs:258-298).  They are the inverse of writers.leaflets_export_text / normals_export_text
and give the arrays HipEngine.set_manual_leaflet_table / set_manual_normal_table take.

Both files are a YAML mapping from a molecule type's name to a sequence with one flow list per row (assignment frame, or
analysed frame), comments between them; nothing else of YAML is used, so they are read without a YAML library."""
import json
from typing import Dict, List

import numpy as np


def _rows_per_type(text: str) -> Dict[str, List[list]]:
    rows: Dict[str, List[list]] = {}
    current = None
    for number, raw in enumerate(text.splitlines(), start=1):
        line = raw.split("#", 1)[0].rstrip()
        if not line.strip():
            continue
        if not line[0].isspace() and line.endswith(":"):
            current = line[:-1].strip().strip("'\"")
            if current in rows:
                raise ValueError(f"line {number}: molecule type {current!r} appears twice")
            rows[current] = []
        elif line.lstrip().startswith("- ") and current is not None:
            try:
                rows[current].append(json.loads(line.lstrip()[2:]))       # (json reads NaN as the writer spells it)
            except ValueError as e:
                raise ValueError(f"line {number}: not a flow list: {e}") from None
        else:
            raise ValueError(f"line {number}: neither a molecule type nor a row: {raw!r}")
    return rows


def _columns(text: str, labels, what: str):
    rows = _rows_per_type(text)
    missing = [m.name for m in labels if m.name not in rows]
    if missing:
        raise ValueError(f"the {what} file has no molecule type {missing[0]!r}")      # MoleculeNotFound
    n_rows = {len(rows[m.name]) for m in labels}
    if len(n_rows) > 1:
        raise ValueError(f"the molecule types of the {what} file have different numbers of rows: {sorted(n_rows)}")
    return [rows[m.name] for m in labels], (n_rows.pop() if n_rows else 0)


def read_leaflets_file(text: str, labels) -> np.ndarray:
    """A leaflet assignment file -> flags [rows, n_molecules_total] uint8 in this repo's encoding (Upper = 0, Lower = 1; the
    file holds 1 = upper, 0 = lower), molecules molecule-type-major in the order of `labels` (objects with .name and
    .n_molecules, as structure.build_tables returns).  Row r is the assignment of frames [r * frequency, (r + 1) * frequency)."""
    per_type, n_rows = _columns(text, labels, "leaflet assignment")
    out = np.zeros((n_rows, sum(m.n_molecules for m in labels)), dtype=np.uint8)
    at = 0
    for m, rows in zip(labels, per_type):
        for r, row in enumerate(rows):
            if len(row) != m.n_molecules or any(x not in (0, 1) for x in row):
                raise ValueError(f"{m.name}, row {r}: expected {m.n_molecules} values of 0 or 1")
            out[r, at:at + m.n_molecules] = 1 - np.asarray(row, dtype=np.uint8)
        at += m.n_molecules
    return out


def read_normals_file(text: str, labels) -> np.ndarray:
    """A membrane normals file -> normals [rows, n_molecules_total, 3] float32, molecules as above; row r belongs to the r-th
    analysed frame.  A vector the writer spelled NaN stays NaN."""
    per_type, n_rows = _columns(text, labels, "membrane normals")
    out = np.zeros((n_rows, sum(m.n_molecules for m in labels), 3), dtype=np.float32)
    at = 0
    for m, rows in zip(labels, per_type):
        for r, row in enumerate(rows):
            try:
                a = np.asarray(row, dtype=np.float64)
            except (ValueError, TypeError):           # ragged: some vector has no 3 components
                a = np.zeros(0)
            if a.shape != (m.n_molecules, 3):
                raise ValueError(f"{m.name}, row {r}: expected {m.n_molecules} vectors of 3 components")
            out[r, at:at + m.n_molecules] = a
        at += m.n_molecules
    return out
