"""Text output in the reference's layouts, from the result tree of `structure.results_tree[_ua]`:
YAML (presentation/yaml_presenter.rs:80-136: nested mapping, values rounded to 4 decimals, NaN as `.nan`) and CSV
(presentation/csv_presenter.rs: one line per heavy atom or coarse-grained bond, fixed 4 decimals, NaN as `NaN`, empty
fields for hydrogens an atom does not have).  Both can be compared with the reference's files by its own rule
(tests/common/mod.rs:95-150: same items line by line, numbers within 2e-4).  Ordermaps: the `.dat` files and the directory
tree of presentation/ordermaps_presenter.rs, from the values of `HipEngine.ordermaps` / `structure.ordermap_values`."""
import os
import re
from typing import List, Optional


def _num(x) -> str:
    if x != x:
        return ".nan"
    s = repr(float(x))
    return s[:-2] if s.endswith(".0") else s


def yaml_text(tree: dict, header: Optional[str] = None) -> str:
    out: List[str] = [header] if header else []

    def emit(node, indent):
        pad = "  " * indent
        for key, val in node.items():
            if isinstance(val, dict):
                out.append(f"{pad}{key}:")
                emit(val, indent + 1)
            elif isinstance(val, (list, tuple)):       # united atoms: `bonds:` is a sequence of mappings
                out.append(f"{pad}{key}:")
                for item in val:
                    first = True
                    for k2, v2 in item.items():
                        lead = f"{pad}- " if first else f"{pad}  "
                        first = False
                        if isinstance(v2, dict):
                            out.append(f"{lead}{k2}:")
                            emit(v2, indent + 2)
                        else:
                            out.append(f"{lead}{k2}: {_num(v2)}")
            else:
                out.append(f"{pad}{key}: {_num(val)}")

    emit(tree, 0)
    return "\n".join(out) + "\n"


_ATOM_KEY = re.compile(r"^(\S+) (\S+) \((\d+)\)$")
_BOND_KEY = re.compile(r"^(\S+) (\S+) \((\d+)\) - (\S+) (\S+) \((\d+)\)$")


def _fixed(x) -> str:
    return "NaN" if x != x else f"{x:.4f}"


def _cells(value: dict, which: List[str], errors: bool) -> List[str]:
    """One order parameter as CSV cells: per leaflet slot the mean (and its error)."""
    cells = []
    for w in which:
        v = value[w]
        if errors:
            cells += [_fixed(v["mean"]), _fixed(v["error"])]
        else:
            cells.append(_fixed(v))
    return cells


def csv_text(tree: dict) -> str:
    """AA / UA: molecule,residue,atom,relative index,total…,hydrogen #k…   CG: molecule,atom 1,atom 2,…"""
    molecules = [(k, v) for k, v in tree.items() if k != "average order"]
    sample = tree["average order"]
    which = [w for w in ("total", "upper", "lower") if w in sample]
    leaflets = len(which) == 3
    errors = isinstance(sample["total"], dict)
    first_op = next(iter(molecules[0][1]["order parameters"].values()))
    atom_based = "bonds" in first_op
    suffix = {"total": " full membrane", "upper": " upper leaflet", "lower": " lower leaflet"}

    def columns(name: str) -> List[str]:
        cols = []
        for w in which:
            label = (name + suffix[w]) if leaflets else name
            cols.append(label)
            if errors:
                cols.append(label + " error")
        return cols

    lines = []
    if atom_based:
        n_h = 0
        for _, mol in molecules:
            for entry in mol["order parameters"].values():
                n_h = max(n_h, len(entry["bonds"]))
        head = ["molecule", "residue", "atom", "relative index"] + columns("total")
        for k in range(n_h):
            head += columns(f"hydrogen #{k + 1}")
        lines.append(",".join(head))
        width = len(columns("x"))
        for mname, mol in molecules:
            for key, entry in mol["order parameters"].items():
                res, atom, rel = _ATOM_KEY.match(key).groups()
                row = [mname, res, atom, rel] + _cells(entry, which, errors)
                bonds = entry["bonds"]
                bonds = list(bonds.values()) if isinstance(bonds, dict) else list(bonds)
                for k in range(n_h):
                    row += _cells(bonds[k], which, errors) if k < len(bonds) else [""] * width
                lines.append(",".join(row))
    else:
        def cg_columns():
            cols = []
            for w in which:
                label = suffix[w].strip()
                cols.append(label)
                if errors:
                    cols.append(label + " error")
            return cols
        lines.append(",".join(["molecule", "atom 1", "atom 2"] + cg_columns()))
        for mname, mol in molecules:
            for key, entry in mol["order parameters"].items():
                _, a1, _, _, a2, _ = _BOND_KEY.match(key).groups()
                lines.append(",".join([mname, a1, a2] + _cells(entry, which, errors)))
    return "\n".join(lines) + "\n"


def _pm(value, errors: bool) -> str:
    if errors:
        if value["mean"] != value["mean"]:             # tab_presenter.rs:135-139: one centred NaN, no error beside it
            return f"{'NaN':^17s}"
        return f"{_fixed(value['mean']):>8s} ± {_fixed(value['error'])}"
    return f"{_fixed(value):>8s}"


def tab_text(tree: dict, header: Optional[str] = None) -> str:
    """The table layout (presentation/tab_presenter.rs): per molecule type one row per heavy atom (TOTAL and the
    hydrogens) or per coarse-grained bond, an AVERAGE row, and the average of all molecule types at the end.  The
    reference compares these files token by token (tests/common/mod.rs:113-124), so column widths are cosmetic."""
    molecules = [(k, v) for k, v in tree.items() if k != "average order"]
    sample = tree["average order"]
    which = [w for w in ("total", "upper", "lower") if w in sample]
    leaflets = len(which) == 3
    errors = isinstance(sample["total"], dict)
    atom_based = "bonds" in next(iter(molecules[0][1]["order parameters"].values()))
    out = [header or "# order parameters", ""]
    slot_names = "      ".join(("FULL", "UPPER", "LOWER")) if leaflets else None

    def cell(value) -> str:
        return "   ".join(_pm(value[w], errors) for w in which)

    def head_rows(groups: List[str], label: str):
        if atom_based and not (leaflets and groups == ["TOTAL"] and label == "all"):
            out.append(" " * 10 + "  |  ".join(f"{g:^{len(cell(sample))}s}" for g in groups) + "  |")
        if leaflets:
            out.append(" " * 10 + "  |  ".join(slot_names for _ in groups) + "  |")
        elif not atom_based:
            out.append(" " * 18 + "FULL   |")

    for mname, mol in molecules:
        out.append(f"Molecule type {mname}")
        ops = mol["order parameters"]
        if atom_based:
            n_h = max(len(e["bonds"]) for e in ops.values())
            hname = "HYDROGEN" if (leaflets or errors) else "H"      # the narrow table abbreviates
            head_rows(["TOTAL"] + [f"{hname} #{k + 1}" for k in range(n_h)], "mol")
            for key, entry in ops.items():
                atom = _ATOM_KEY.match(key).group(2)
                bonds = entry["bonds"]
                bonds = list(bonds.values()) if isinstance(bonds, dict) else list(bonds)
                cells = [cell(entry)] + [cell(bonds[k]) if k < len(bonds) else " " * len(cell(entry)) for k in range(n_h)]
                out.append(f"{atom:<8s}" + "  |  ".join(cells) + "  |")
        else:
            head_rows(["FULL"], "mol")
            for key, entry in ops.items():
                _, a1, _, _, a2, _ = _BOND_KEY.match(key).groups()
                out.append(f"{a1 + ' - ' + a2:<15s}" + cell(entry) + "  |")
        out.append(f"{'AVERAGE':<8s}" + cell(mol["average order"]) + "  |")
        out.append("")
    out.append("All molecule types")
    head_rows(["TOTAL"] if atom_based else ["FULL"], "all")
    out.append(f"{'AVERAGE':<8s}" + cell(sample) + "  |")
    return "\n".join(out) + "\n"


def xvg_text(tree: dict, molecule: str, header: Optional[str] = None, united: bool = False) -> str:
    """One molecule type as an xvg data set (presentation/xvg_presenter.rs): a numbered line per heavy atom / bond,
    full membrane and, with leaflets, upper and lower."""
    mol = tree[molecule]
    ops = mol["order parameters"]
    sample = tree["average order"]
    which = [w for w in ("total", "upper", "lower") if w in sample]
    errors = isinstance(sample["total"], dict)
    atom_based = "bonds" in next(iter(ops.values()))
    out = [header or "# order parameters",
           f'@    title "{("United-atom" if united else "Atomistic") if atom_based else "Coarse-grained"} order parameters for molecule type {molecule}"',
           f'@    xaxis label "{"Atom" if atom_based else "Bond"}"',
           f'@    yaxis label "{"-Sch" if atom_based else "S"}"']
    legends = {"total": "Full membrane", "upper": "Upper leaflet", "lower": "Lower leaflet"}
    for k, w in enumerate(which):
        out.append(f'@    s{k} legend "{legends[w]}"')
    out.append("@TYPE xy")
    for n, (key, entry) in enumerate(ops.items(), start=1):
        if atom_based:
            out.append(f"# Atom {_ATOM_KEY.match(key).group(2)}:")
        else:
            _, a1, _, _, a2, _ = _BOND_KEY.match(key).groups()
            out.append(f"# Bond {a1} - {a2}:")
        vals = [entry[w]["mean"] if errors else entry[w] for w in which]
        out.append(f"{n:<4d} " + " ".join(f"{_fixed(v):>8s}" for v in vals) + " ")
    return "\n".join(out) + "\n"


def convergence_groups(labels) -> list:
    """The slots of every molecule type, in the order of the labels: the groups whose running averages convergence_text
    prints (what HipEngine.convergence takes as `groups`)."""
    out = []
    for ml in labels:
        n_slots = sum(c.n_h for c in ml.carbons) if hasattr(ml, "carbons") else len(ml.bonds)
        out.append(list(range(ml.slot0, ml.slot0 + n_slots)))
    return out


def _prefix_columns(timewise, groups, leaflets: bool = True):
    """prefix [frames][3][n_groups] float32 from the rows: cumulative tick sum / cumulative sample count by the truncating
    integer division, / 1e6 as f32; NaN while nothing was sampled (without `leaflets` only [:, 0] is filled in).  (The device's gorder_hip_convergence makes the same.)"""
    import numpy as np
    sums, counts = (np.asarray(x) for x in timewise)
    prefix = np.full((sums.shape[0], 3, len(groups)), np.nan, dtype=np.float32)
    for g, slots in enumerate(groups):
        for w in range(3 if leaflets else 1):
            cs = np.cumsum(sums[:, w, slots].sum(axis=1).astype(np.int64))
            cn = np.cumsum(counts[:, w, slots].sum(axis=1).astype(np.int64))
            for f, (s_, n_) in enumerate(zip(cs, cn)):
                if n_ != 0:
                    q = abs(int(s_)) // int(n_)
                    prefix[f, w, g] = np.float32((-q if s_ < 0 else q) / 1e6)
    return prefix


def convergence_text(timewise, labels, analysis: str, leaflets: bool, header: Optional[str] = None, step: int = 1,
                     prefix=None) -> str:
    """Convergence of the molecule types' average order parameters (TimeWiseData::prefix_average, timewise.rs:259-274;
    presentation/convergence.rs): line n holds, per molecule type (and leaflet), the average over the first n analysed
    frames — cumulative tick sum / cumulative sample count by the truncating integer division, sign as in the
    other outputs.  `timewise` = (sums, counts) [frames][3][n_acc] as returned by the engines; `labels` as from
    build_tables*; x = the frame's number in the trajectory, 1 + n * step.
    prefix [frames][3][n_molecule_types] (HipEngine.convergence(convergence_groups(labels))): the columns made on the
    device, in place of `timewise` (which may then be None)."""
    import numpy as np
    if prefix is None:
        prefix = _prefix_columns(timewise, convergence_groups(labels), leaflets)
    prefix = np.asarray(prefix)
    sign = -1.0 if analysis in ("aa", "ua") else 1.0
    which = ["full", "upper", "lower"] if leaflets else [""]
    out = [header or "# order parameters",
           '@    title "Convergence of average order parameters for individual molecule types"',
           '@    xaxis label "Frame number"',
           f'@    yaxis label "{"-Sch" if analysis in ("aa", "ua") else "S"}"']
    cols = []
    for g, ml in enumerate(labels):
        for w, name in enumerate(which):
            out.append(f'@    s{len(cols)} legend "{(ml.name + " " + name).strip()}"')
            cols.append([float("nan") if v != v else sign * float(v) for v in prefix[:, w, g]])
    out.append("@TYPE xy")
    for f in range(prefix.shape[0]):
        out.append(f"{f * step + 1:<4d} " + " ".join(f"{_fixed(c[f]):>8s}" for c in cols) + " ")
    return "\n".join(out) + "\n"


def _per_type_rows(labels, n_columns: int):
    """(name, column slice) per molecule type: the molecules are stored molecule type major."""
    at = 0
    for ml in labels:
        yield ml.name, slice(at, at + ml.n_molecules)
        at += ml.n_molecules
    if at != n_columns:
        raise ValueError(f"the labels hold {at} molecules, the rows {n_columns}")


def leaflets_export_text(flags, frames, labels, frequency: int, header: Optional[str] = None) -> str:
    """The reference's leaflet assignment file (tests/golden/expected/aa_leaflets_every5.yaml) from what
    HipEngine.collected_leaflets returns: per molecule type a sequence with one flow list per assignment frame, 1 = upper
    and 0 = lower (this repo stores Upper = 0), each under a comment with the frame's number counted from 1.  `frequency`
    is the real frequency of the classifier (0 = once): the frames must be its assignment frames."""
    import numpy as np
    flags, frames = np.asarray(flags), np.asarray(frames)
    if flags.ndim != 2 or len(frames) != flags.shape[0]:
        raise ValueError("flags [rows, molecules] and frames [rows]")
    for f in frames:
        if (int(f) != 0) if frequency == 0 else (int(f) % frequency != 0):
            raise ValueError(f"frame {int(f)} is not an assignment frame of frequency {frequency}")
    out = [header or "# Leaflet assignment file"]
    for name, cols in _per_type_rows(labels, flags.shape[1]):
        out.append(f"{name}:")
        for row, f in zip(flags, frames):
            out.append(f"# Frame index {int(f) + 1}")
            out.append("  - [" + ",".join("0" if x else "1" for x in row[cols]) + "]")
    return "\n".join(out) + "\n"


def _component(x) -> str:
    return f"{'NaN' if x != x else format(float(x), '.6f'):>9s}"


def normals_export_text(normals, frames, labels, header: Optional[str] = None) -> str:
    """The reference's membrane normals file (tests/golden/expected/ua_normals.yaml) from what
    HipEngine.collected_normals returns: per molecule type one flow list of [x,y,z] per analysed frame, every component
    9 wide with 6 decimals, a normal that was never computed as NaN (a YAML reader takes that as a string: read it back
    with float())."""
    import numpy as np
    normals, frames = np.asarray(normals), np.asarray(frames)
    if normals.ndim != 3 or normals.shape[2] != 3 or len(frames) != normals.shape[0]:
        raise ValueError("normals [rows, molecules, 3] and frames [rows]")
    out = [header or "# Membrane normals file"]
    for name, cols in _per_type_rows(labels, normals.shape[1]):
        out.append(f"{name}:")
        for row, f in zip(normals, frames):
            out.append(f"# Frame index {int(f) + 1}")
            out.append("  - [" + ",".join("[" + ",".join(_component(c) for c in v) + "]" for v in row[cols]) + "]")
    return "\n".join(out) + "\n"


def radial_profile_text(values, counts, radii, names, header: Optional[str] = None) -> str:
    """A radial profile as text (this project's own layout: the reference has no such file), from the values
    [n_groups, 3, n_shells] of structure.radial_profile, the radii given to HipEngine.set_radial_shells and one name per
    group: one row per shell — `r_inner r_outer` in nm, then per group its full, upper and lower value with four decimals,
    NaN as `NaN` — under `#` lines that name the columns.  counts [n_groups, 3, n_shells] (structure.radial_counts), or
    None: with them every group gets a fourth column, the samples behind its full value."""
    if len(values) != len(names) or any(len(w) != len(radii) for v in values for w in v):
        raise ValueError("values [n_groups, 3, n_shells], one name per group, one radius per shell")
    if counts is not None and (len(counts) != len(names) or any(len(c[0]) != len(radii) for c in counts)):
        raise ValueError("counts [n_groups, 3, n_shells]")
    out = [header or "# radial profile of order parameters",
           "# shell k holds the samples at distance r_inner <= d < r_outer [nm] from the reference of the selection",
           "# column 1: r_inner", "# column 2: r_outer"]
    col = 3
    for name in names:
        for which in ("full", "upper", "lower") + (("samples",) if counts is not None else ()):
            out.append(f"# column {col}: {name} {which}")
            col += 1
    for k, r in enumerate(radii):
        cells = [_fixed(float(radii[k - 1]) if k else 0.0), _fixed(float(r))]
        for g in range(len(names)):
            cells += [f"{_fixed(float(values[g][w][k])):>8s}" for w in range(3)]
            if counts is not None:
                cells.append(str(int(counts[g][0][k])))
        out.append(" ".join(cells))
    return "\n".join(out) + "\n"


def class_profile_text(values, counts, names, header: Optional[str] = None) -> str:
    """Order parameters by number of neighbours as text (this project's own layout: the reference has no such file), from the
    values [n_groups, 3, n_classes] of structure.class_profile and one name per group: one line per class — the number of
    neighbours, the last class labelled `>= n - 1` —, then per group its full, upper and lower value with four decimals, NaN as
    `NaN`, under `#` lines that name the columns.  counts [n_groups, 3, n_classes] (structure.class_counts), or None: with
    them every group gets a fourth column, the samples behind its full value."""
    n_classes = len(values[0][0]) if len(values) else 0
    if len(values) != len(names) or any(len(w) != n_classes for v in values for w in v):
        raise ValueError("values [n_groups, 3, n_classes], one name per group")
    if counts is not None and (len(counts) != len(names) or any(len(c[0]) != n_classes for c in counts)):
        raise ValueError("counts [n_groups, 3, n_classes]")
    out = [header or "# order parameters by number of neighbours",
           "# class k holds the samples of molecules with k neighbour atoms within the radius of their centre, the last class that many or more",
           "# column 1: neighbours"]
    col = 2
    for name in names:
        for which in ("full", "upper", "lower") + (("samples",) if counts is not None else ()):
            out.append(f"# column {col}: {name} {which}")
            col += 1
    for k in range(n_classes):
        cells = [f">={k}" if k == n_classes - 1 else str(k)]
        for g in range(len(names)):
            cells += [f"{_fixed(float(values[g][w][k])):>8s}" for w in range(3)]
            if counts is not None:
                cells.append(str(int(counts[g][0][k])))
        out.append(" ".join(cells))
    return "\n".join(out) + "\n"


def molecule_order_text(values, frames, names, header: Optional[str] = None) -> str:
    """Per-molecule order parameters as text (this project's own layout: the reference has no such file), from the values
    [rows, n_groups, n_molecules] of structure.molecule_order, the frames of HipEngine.molecule_rows and one name per group:
    one line per frame — the frame's global index, then group by group every molecule's value with four decimals, NaN as
    `NaN` (a molecule that is not of the group's type, or below min_samples) — under `#` lines that name the columns."""
    if len(values) != len(frames) or any(len(v) != len(names) for v in values):
        raise ValueError("values [rows, n_groups, n_molecules], one frame index per row, one name per group")
    n_mol = len(values[0][0]) if len(values) and len(names) else 0
    out = [header or "# order parameters of single molecules, frame by frame", "# column 1: frame index"]
    for g, name in enumerate(names):
        out.append(f"# columns {2 + g * n_mol}-{1 + (g + 1) * n_mol}: {name}, molecules 0-{n_mol - 1}")
    for row, f in zip(values, frames):
        out.append(" ".join([str(int(f))] + [_fixed(float(x)) for grp in row for x in grp]))
    return "\n".join(out) + "\n"


def order_histogram_text(counts, edges, names, angles=None, header: Optional[str] = None) -> str:
    """An order distribution as text (this project's own layout: the reference has no such file), from the counts
    [n_groups, 3, n_bins] of structure.histogram_groups, the tick edges given to HipEngine.set_order_histogram and one name
    per group: one row per bin — `tick_low tick_high`, the bin edges[k] <= 1e6 S < edges[k + 1] of the raw S =
    1.5 cos^2 - 0.5 as integers, with `angles` (structure.tilt_edges) the bin's two tilt angles in degrees with four
    decimals behind them — then per group its full, upper and lower sample count, under `#` lines that name the columns."""
    n_bins = len(edges) - 1
    if len(counts) != len(names) or any(len(w) != n_bins for c in counts for w in c):
        raise ValueError("counts [n_groups, 3, n_bins], one name per group, n_bins + 1 edges")
    if angles is not None and len(angles) != len(edges):
        raise ValueError("one angle per edge")
    out = [header or "# distribution of order parameters: samples per bin",
           "# bin k holds the samples with tick_low <= 1e6 * S < tick_high, S = 1.5 cos^2(theta) - 0.5 of the bond vector",
           "# column 1: tick_low", "# column 2: tick_high"]
    col = 3
    if angles is not None:
        out += ["# column 3: theta at tick_low [deg]", "# column 4: theta at tick_high [deg]"]
        col = 5
    for name in names:
        for which in ("full", "upper", "lower"):
            out.append(f"# column {col}: {name} {which}")
            col += 1
    for k in range(n_bins):
        cells = [str(int(edges[k])), str(int(edges[k + 1]))]
        if angles is not None:
            cells += [_fixed(float(angles[k])), _fixed(float(angles[k + 1]))]
        for g in range(len(names)):
            cells += [str(int(counts[g][w][k])) for w in range(3)]
        out.append(" ".join(cells))
    return "\n".join(out) + "\n"


def bond_correlation_text(values, lags, names, dt: float = 1.0, header: Optional[str] = None) -> str:
    """A bond reorientation correlation as text (this project's own layout: the reference has no such file), from the values
    [n_groups, 3, n_lags] of structure.correlation_values, the lags given to HipEngine.set_bond_correlation and one name per
    group: one row per lag — the lag in analysed frames, the lag times `dt` with four decimals — then per group its full,
    upper and lower C(lag) with six decimals (NaN as `NaN`), under `#` lines that name the columns."""
    n_lags = len(lags)
    if len(values) != len(names) or any(len(w) != n_lags for v in values for w in v) or any(len(v) != 3 for v in values):
        raise ValueError("values [n_groups, 3, n_lags], one name per group, one lag per column")
    out = [header or "# bond reorientation: C(lag) = <P2(u(t) . u(t + lag))> over t and the molecules",
           "# column 1: lag [analysed frames]", "# column 2: lag * dt"]
    col = 3
    for name in names:
        for which in ("full", "upper", "lower"):
            out.append(f"# column {col}: {name} {which}")
            col += 1
    for k in range(n_lags):
        cells = [str(int(lags[k])), _fixed(float(lags[k]) * float(dt))]
        for g in range(len(names)):
            for w in range(3):
                x = float(values[g][w][k])
                cells.append("NaN" if x != x else f"{x:.6f}")
        out.append(" ".join(cells))
    return "\n".join(out) + "\n"


_PLANE_LABELS = {0: ("x", "y"), 1: ("x", "z"), 2: ("z", "y")}     # Plane::get_labels (input/ordermap.rs:54-60)
_LEAFLET_NAMES = ("full", "upper", "lower")


def ordermap_text(values, ordermap, analysis: str, comment: str, calculated_with: str = "gorder_amd") -> str:
    """One ordermap file (write_ordermap, presentation/ordermaps_presenter.rs:352-385) from the values [nx, ny] of one group
    and plane: `comment` (the line ordermap_groups gives) and the line naming the program, the axis labels of the plane, the
    z label and range of the analysis type, then `x y value` per tile, x-major, four decimals, NaN as `NaN`.  A tile sits at
    span minimum + index * bin."""
    import numpy as np
    v = np.asarray(values, dtype=np.float32)
    if v.ndim != 2:
        raise ValueError("values [nx, ny] of one map")
    atomistic = analysis in ("aa", "ua")
    lx, ly = _PLANE_LABELS[int(ordermap.plane)]
    head = [comment, f"# Calculated with '{calculated_with}'.",
            f"@ xlabel {lx}-dimension [nm]", f"@ ylabel {ly}-dimension [nm]",
            "@ zlabel order parameter ($-S_{CH}$)" if atomistic else "@ zlabel order parameter ($S$)",
            "@ zrange -1.0 0.5 0.25" if atomistic else "@ zrange -0.5 1.0 0.25",
            "$ type colorbar", "$ colormap seismic_r"]
    if v.size == 0:
        return "\n".join(head) + "\n"
    x = np.char.mod("%.4f", ordermap.span_x[0] + np.arange(v.shape[0]) * ordermap.bin[0])
    y = np.char.mod("%.4f", ordermap.span_y[0] + np.arange(v.shape[1]) * ordermap.bin[1])
    flat = v.ravel().astype(np.float64)
    z = np.where(np.isnan(flat), "NaN", np.char.mod("%.4f", flat))
    lines = np.char.add(np.char.add(np.repeat(x, v.shape[1]), " "), np.char.add(np.char.add(np.tile(y, v.shape[0]), " "), z))
    return "\n".join(head) + "\n" + "\n".join(lines.tolist()) + "\n"


def write_ordermaps(directory, values, groups, ordermap, analysis: str, leaflets: bool, calculated_with: str = "gorder_amd") -> list:
    """The reference's ordermap directory (OrderMapPresenter::write, presentation/ordermaps_presenter.rs:110-322) from
    values [n_groups, 3, nx, ny] and the groups of structure.ordermap_groups: the maps of the whole system at the top, a
    directory per molecule type with its average, atom and bond maps, each as `_full` and, with leaflets, `_upper` and
    `_lower`.  The reference's plotting script is not written.  Returns the paths written, relative to `directory`."""
    if len(values) != len(groups):
        raise ValueError(f"{len(values)} maps for {len(groups)} groups")
    written = []
    os.makedirs(directory, exist_ok=True)
    for vals, group in zip(values, groups):
        for sub, stem, comment in group.files:
            if sub:
                os.makedirs(os.path.join(directory, sub), exist_ok=True)
            for w in range(3 if leaflets else 1):
                rel = os.path.join(sub, f"{stem}_{_LEAFLET_NAMES[w]}.dat")
                with open(os.path.join(directory, rel), "w") as f:
                    f.write(ordermap_text(vals[w], ordermap, analysis, comment, calculated_with))
                written.append(rel)
    return written
