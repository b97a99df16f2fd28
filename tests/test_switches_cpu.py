"""The development switches (gorder_amd/csrc/switches.h) without a GPU: a stand-alone program under the address and
undefined-behaviour sanitizers reads them from an environment given on its command line and prints every member of
gorder::Switches and how often each name was looked up.  The expected values here restate the expressions of the sites that
read the environment before the header existed (commit 9c87605: gorder_hip.hip — env_flag, create_accumulators,
create_spherical, gorder_hip_create, launch_map_accumulate —, local_slab_frames in kernels_leaflets.h, run_trajectory in
trajectory_driver.h), not the header.  The header's table is also the documentation's: the names in include/gorder_hip.h,
DESIGN.md and the comments of the other sources are the table's."""
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gorder_amd", "csrc")
NAME = re.compile(r"GORDER_HIP_[A-Z0-9_]+")


def atoi(v):
    """atoi / atol / atoll on the values used here (all far inside an int): leading white space, a sign, digits; else 0"""
    m = re.match(r"\s*([+-]?\d+)", v)
    return int(m.group(1)) if m else 0


def flag(v):                            # env_flag: set, non-empty, not the string "0"
    return int(v != "" and v != "0")


def keep_if(ok, default):               # `if (ok(v)) field = v;` on a field that holds `default`
    return lambda v: atoi(v) if ok(atoi(v)) else default


GIB = 1 << 30
# name -> (member, value when the variable is not set, value when it is set to the string v)
PARENT = {
    "GORDER_HIP_KERNEL": ("kernel_gather", 0, lambda v: int(v == "gather")),
    "GORDER_HIP_WG_TARGET": ("wg_target", 0, keep_if(lambda w: w > 0, 0)),
    "GORDER_HIP_NPF5": ("npf5", 0, flag),
    "GORDER_HIP_TW_GATHER": ("tw_gather", 0, flag),
    "GORDER_HIP_MAPS_GATHER": ("maps_gather", 0, flag),
    "GORDER_HIP_FORCE_DIRECT": ("force_direct", 0, flag),
    "GORDER_HIP_UA_SLOT_WAVES": ("ua_slot_waves", 0, flag),
    "GORDER_HIP_REPLICAS": ("replicas", 32, keep_if(lambda r: 1 <= r <= 1024, 32)),
    "GORDER_HIP_MAP_DIRECT": ("map_direct", 0, flag),
    "GORDER_HIP_MAP_CHUNKS": ("map_chunks", 0, lambda v: max(1, atoi(v))),
    "GORDER_HIP_MAP_FOLD_LIMIT": ("map_fold_limit", 0, atoi),      # as written: the range [2, kMapFoldLimit] is tested where it is used
    "GORDER_HIP_NO_SPECULATE": ("no_speculate", 0, flag),
    "GORDER_HIP_LEAFLETS_GENERIC": ("leaflets_generic", 0, flag),
    "GORDER_HIP_SPHERICAL_SLAB": ("spherical_slab", 0, lambda v: max(1, atoi(v))),
    "GORDER_HIP_CLUSTER_STORED_W": ("cluster_stored_w", 0, flag),
    "GORDER_HIP_LOCAL_SLAB": ("local_slab", 0, lambda v: max(4, atoi(v))),
    "GORDER_HIP_LOCAL_ATOMS_ONLY": ("local_atoms_only", 0, flag),
    "GORDER_HIP_LOCAL_THREE_KERNELS": ("local_three_kernels", 0, flag),
    "GORDER_HIP_LOCAL_NO_DECIDE": ("local_no_decide", 0, flag),
    "GORDER_HIP_LOCAL_NO_SUMS": ("local_no_sums", 0, flag),
    "GORDER_HIP_LOCAL_NO_PRUNE": ("local_no_prune", 0, flag),
    "GORDER_HIP_LOCAL_DECIDE_NOTHING": ("local_decide_nothing", 0, flag),
    "GORDER_HIP_RADIAL_DIRECT": ("radial_direct", 0, flag),
    "GORDER_HIP_DIST_DIRECT": ("dist_direct", 0, flag),
    "GORDER_HIP_DIST_SAMPLES_PER_WORD": ("dist_samples_per_word", 8, lambda v: min(max(0, atoi(v)), 1 << 16)),
    "GORDER_HIP_NB_DIRECT": ("nb_direct", 0, flag),
    "GORDER_HIP_NB_SUBRANGE": ("nb_subrange", 0, lambda v: max(0, atoi(v))),
    "GORDER_HIP_NB_ROW_BYTES": ("nb_row_bytes", GIB, keep_if(lambda b: b > 0, GIB)),
    "GORDER_HIP_CORR_SUBRANGE": ("corr_subrange", 0, lambda v: max(0, atoi(v))),
    "GORDER_HIP_CORR_GRID": ("corr_grid_chunks", 0, lambda v: int(v == "chunks")),
    "GORDER_HIP_MOL_ROWS_STAGING": ("mol_rows_staging", GIB, keep_if(lambda b: b > 0, GIB)),
    "GORDER_HIP_PREFIX_Q16": ("prefix_q16", 0, lambda v: max(1, min(65536, atoi(v)))),
    "GORDER_HIP_NO_PREFIX": ("no_prefix", 0, flag),
}
# every switch is read at every one of these: the values every switch must take, then one inside each clamp, the one at each
# clamp's edge and the one past it (REPLICAS 0 1 1024 1025; MAP_FOLD_LIMIT 1 2; DIST_SAMPLES_PER_WORD 65536 65537; LOCAL_SLAB
# 3 4; PREFIX_Q16 0 1 65536 65537; MAP_CHUNKS, SPHERICAL_SLAB 0 1 2; the SUBRANGEs -1 0 3; the byte bounds -1 0 1), the words
# of KERNEL and CORR_GRID and their near misses, and what a flag must not take for "0".  (A value past 32 bits goes to the two
# byte bounds alone, below: they are read with atoll, and atoi of such a value is nobody's to define.)
VALUES = ["", "0", "1", "-3", "abc",
          "2", "3", "4", "5", "7", "16", "40", "250", "1024", "1025", "2000", "65535", "65536", "65537", "-1", "1000",
          "2097152", "2097153", " 12", "+9", "12abc",
          "gather", "Gather", "chunks", "tiles", "00", "no"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("switches") / "switches")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", f"-I{CSRC}", os.path.join(ROOT, "tests", "cabi", "switches.cpp"), "-o", exe])

    def run(env=None):
        """no env: the table's (name, meaning) pairs; else (member -> value, name -> lookups)"""
        args = [] if env is None else [f"{k}={v}" for k, v in env.items()] or ["GORDER_NOT_A_SWITCH=1"]
        res = subprocess.run([exe, *args], capture_output=True, timeout=60)
        err = res.stderr.decode()
        assert res.returncode == 0 and "Sanitizer" not in err and "runtime error" not in err, err
        lines = res.stdout.decode().splitlines()
        if env is None:
            return [tuple(line.split("\t")) for line in lines]
        members = {m: int(v) for m, v in (line.split() for line in lines if not line.startswith("lookup "))}
        lookups = {line.split()[1]: int(line.split()[2]) for line in lines if line.startswith("lookup ")}
        assert len(members) + len(lookups) == len(lines)
        return members, lookups
    return run


def test_the_table_is_the_parents_set_of_names(driver):
    table = driver()
    assert all(len(row) == 2 and row[1] for row in table)
    names = [name for name, _ in table]
    assert len(names) == len(set(names)) == 33 and set(names) == set(PARENT)
    assert len({member for member, _, _ in PARENT.values()}) == len(PARENT)


def test_defaults(driver):
    members, lookups = driver({})
    assert members == {member: default for member, default, _ in PARENT.values()}
    assert lookups == {name: 1 for name in PARENT}


@pytest.mark.parametrize("value", VALUES)
def test_every_switch_parses_as_its_old_reading_site(driver, value):
    members, lookups = driver({name: value for name in PARENT})
    for name, (member, _, parse) in PARENT.items():
        assert members[member] == parse(value), (name, value)
    assert lookups == {name: 1 for name in PARENT}        # each name exactly once per read_switches


def test_byte_bounds_past_32_bits(driver):
    for name in ("GORDER_HIP_NB_ROW_BYTES", "GORDER_HIP_MOL_ROWS_STAGING"):
        members, _ = driver({name: str(8 * GIB)})
        assert members[PARENT[name][0]] == PARENT[name][2](str(8 * GIB)) == 8 * GIB


def test_one_switch_leaves_the_others_at_their_defaults(driver):
    for name, (member, _, parse) in PARENT.items():
        value = {"GORDER_HIP_KERNEL": "gather", "GORDER_HIP_CORR_GRID": "chunks"}.get(name, "5")
        members, lookups = driver({name: value})
        want = {m: d for m, d, _ in PARENT.values()}
        want[member] = parse(value)
        assert want[member] != PARENT[name][1], name         # (the value moves the member)
        assert members == want, name
        assert lookups == {n: 1 for n in PARENT}


def test_the_parents_expressions_at_their_edges():
    """the restatement above, against the numbers the old sites' code gives"""
    assert [atoi(v) for v in ("", "abc", "-3", " 12", "+9", "12abc", "8589934592")] == [0, 0, -3, 12, 9, 12, 8589934592]
    p = {name: parse for name, (_, _, parse) in PARENT.items()}
    assert [p["GORDER_HIP_REPLICAS"](v) for v in ("0", "1", "1024", "1025")] == [32, 1, 1024, 32]
    assert [p["GORDER_HIP_DIST_SAMPLES_PER_WORD"](v) for v in ("-1", "0", "65536", "65537")] == [0, 0, 65536, 65536]
    assert [p["GORDER_HIP_LOCAL_SLAB"](v) for v in ("abc", "3", "4", "5")] == [4, 4, 4, 5]
    assert [p["GORDER_HIP_PREFIX_Q16"](v) for v in ("0", "1", "65536", "65537")] == [1, 1, 65536, 65536]
    assert [p["GORDER_HIP_MAP_CHUNKS"](v) for v in ("", "0", "7")] == [1, 1, 7]
    assert [p["GORDER_HIP_NPF5"](v) for v in ("", "0", "00", "1", "abc")] == [0, 0, 1, 1, 1]


def comment_block(path, title, end):
    """the names from the line with `title` to the first line matching `end` after it"""
    with open(path) as f:
        lines = f.read().splitlines()
    (at,) = [i for i, line in enumerate(lines) if title in line]
    stop = next(i for i in range(at + 1, len(lines)) if re.search(end, lines[i]))
    return NAME.findall("\n".join(lines[at:stop + 1]))


def test_the_list_is_the_documentation(driver):
    names = [name for name, _ in driver()]
    header = comment_block(os.path.join(ROOT, "include", "gorder_hip.h"), "/* Development switches", r"\*/")
    assert header == names                                    # a line per switch, in the table's order
    design = comment_block(os.path.join(ROOT, "DESIGN.md"), "### Development switches", r"^### ")
    assert "GORDER_HIP_LIB" in design
    assert [n for n in design if n != "GORDER_HIP_LIB"] == names
    elsewhere = set()
    for path in sorted(glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.cpp"))):
        if os.path.basename(path) == "switches.h":
            continue
        with open(path) as f:
            for line in f:
                code, _, comment = line.partition("//")
                assert not NAME.search(code) or re.match(r"\s*#\s*(ifndef|define|endif)\b", code), (path, line)     # comments only
                elsewhere.update(NAME.findall(comment))
    assert elsewhere == set(names)
    with open(os.path.join(CSRC, "switches.h")) as f:
        text = f.read()
    assert sorted(NAME.findall(text)) == sorted(names)         # a name is spelled once there


def test_nothing_else_reads_the_environment():
    sites = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        with open(path, errors="replace") as f:
            sites += [(os.path.basename(path), line.strip()) for line in f if "getenv" in line]
    outside = [(name, line) for name, line in sites if name not in ("xtc_reader.cpp", "switches.h")]
    assert len(outside) == 2 and all(name == "gorder_hip.hip" and "read_switches(::getenv)" in line and line.count("getenv") == 1
                                     for name, line in outside), outside
