"""Handcrafted XTC streams and an independent decoder for them (no GPU, no ctypes).

Both decoders of the project — decode_ints in xtc_reader.cpp and k_xtc_scan + k_xtc_chunks in kernels_xtc.h — are
compared with each other everywhere else; this module is the witness outside the pair:

  reference_decode  the published xdr3dcoord decoding in plain Python integers: a bit cursor, `divmod`, nothing else
                    (written from the format description at the top of xtc_reader.cpp, not from its code);
  build_frame       the bytes of one frame from a list of atom groups written AS GIVEN, so that a stream can visit
                    any state of the format, also those no encoder emits;
  families          files of such frames, each with the states it claims to reach (`reached` reads them back from the
                    reference's trace, so a family cannot silently stop reaching its edge).

The format, for a frame of more than 9 atoms: header (magic 1995, natoms, step, time, box, natoms, precision, minint[3],
maxint[3], smallidx, n_bytes), then n_bytes of one MSB-first bit stream, padded to a multiple of 4.  The stream is a
sequence of GROUPS: one full atom (the three numbers coordinate - minint as ONE mixed-radix number with radices
sizeint = maxint - minint + 1 of bit_length(product) bits, or as three fields of bit_length(size) bits when a size
exceeds 0xffffff), one flag bit, with the flag five bits r5 (run = r5 - r5 % 3 numbers follow as run / 3 small atoms;
smallidx moves by r5 % 3 - 1 AFTER the group), without it the run of the group before; then the small atoms, each a
mixed-radix number of `smallidx` bits with radix magic[smallidx] three times, an offset from its predecessor plus
magic[smallidx] / 2.  The first small atom of a run belongs BEFORE the full atom.  A mixed-radix number is stored in
chunks of 8 bits, first chunk least significant, the last (partial) chunk on top.
"""
import struct

import numpy as np

MAGIC = [0, 0, 0, 0, 0, 0, 0, 0, 0, 8, 10, 12, 16, 20, 25, 32, 40, 50, 64, 80, 101, 128, 161, 203, 256, 322, 406, 512,
         645, 812, 1024, 1290, 1625, 2048, 2580, 3250, 4096, 5060, 6501, 8192, 10321, 13003, 16384, 20642, 26007, 32768,
         41285, 52015, 65536, 82570, 104031, 131072, 165140, 208063, 262144, 330280, 416127, 524287, 660561, 832255,
         1048576, 1321122, 1664510, 2097152, 2642245, 3329021, 4194304, 5284491, 6658042, 8388607, 10568983, 13316085,
         16777216]
FIRST_IDX, LAST_IDX = 9, len(MAGIC)          # smallidx lives in [9, 72]
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
MUTANTS = ("no swap", "unflagged resets run", "smallnum after step", "chunks msb first")


class Refused(ValueError):
    """the stream is not a valid frame"""


def field_widths(minint, maxint):
    """-> (sizes, bitsize, three field widths): bitsize 0 = three separate fields"""
    sizes = [int(b) - int(a) + 1 for a, b in zip(minint, maxint)]
    if any(s <= 0 or s > 0xffffffff for s in sizes):
        raise Refused("size of a dimension")
    if max(sizes) > 0xffffff:
        return sizes, 0, [min(s.bit_length(), 32) for s in sizes]
    return sizes, (sizes[0] * sizes[1] * sizes[2]).bit_length(), [0, 0, 0]


# ---- the reference decoder ---------------------------------------------------------------------------------------------
class _Cursor:
    """MSB-first bit cursor over the block: bits [pos, pos + n) of the big-endian integer that the block's bytes spell
    (cut out of the bytes that hold them, which is the same number as shifting the whole block down)"""

    def __init__(self, data, n_bytes=None):
        self.data, self.pos, self.end = bytes(data), 0, 8 * (len(data) if n_bytes is None else n_bytes)

    def read(self, n):
        if n == 0:
            return 0
        if self.pos + n > self.end:
            raise Refused("the stream ends inside a field")
        first, last = self.pos >> 3, (self.pos + n + 7) >> 3
        v = int.from_bytes(self.data[first:last], "big") >> (8 * last - self.pos - n)
        self.pos += n
        return v & ((1 << n) - 1)

    def mixed(self, nbits, sizes, msb_first=False):
        """one mixed-radix number of nbits bits -> its three digits"""
        chunks, left = [], nbits
        while left > 8:
            chunks.append((self.read(8), 8))
            left -= 8
        if left > 0:
            chunks.append((self.read(left), left))
        v, shift = 0, 0
        for c, w in (reversed(chunks) if msb_first else chunks):
            v |= c << shift
            shift += w
        v, c2 = divmod(v, sizes[2])
        c0, c1 = divmod(v, sizes[1])
        return [c0, c1, c2]


def parse_header(buf, pos=0):
    """the frame that starts at buf[pos] -> dict (with `block`, the padded bit stream, and `end`, where the next starts)"""
    if len(buf) < pos + 56:
        raise Refused("short header")
    magic, natoms, step = struct.unpack_from(">iii", buf, pos)
    if magic != 1995:
        raise Refused("magic number")
    h = {"natoms": natoms, "step": step, "time": struct.unpack_from(">f", buf, pos + 12)[0],
         "box": np.array(struct.unpack_from(">9f", buf, pos + 16), np.float32).reshape(3, 3)}
    if struct.unpack_from(">i", buf, pos + 52)[0] != natoms:
        raise Refused("second atom count")
    if natoms <= 9:
        h["raw"] = np.array(struct.unpack_from(">%df" % (3 * natoms), buf, pos + 56), np.float32).reshape(natoms, 3)
        h["end"] = pos + 56 + 12 * natoms
        return h
    h["precision"] = struct.unpack_from(">f", buf, pos + 56)[0]
    six = struct.unpack_from(">6i", buf, pos + 60)
    h["minint"], h["maxint"] = list(six[:3]), list(six[3:])
    h["smallidx"], h["n_bytes"] = struct.unpack_from(">iI", buf, pos + 84)
    padded = (h["n_bytes"] + 3) & ~3
    if len(buf) < pos + 92 + padded:
        raise Refused("the file ends inside the block")
    h["block"] = bytes(buf[pos + 92:pos + 92 + padded])
    h["end"] = pos + 92 + padded
    return h


def reference_decode(frame_bytes, mutant=None):
    """One frame -> (ints int64 [natoms, 3], xyz float32 [natoms, 3], trace).  trace: per group
    (bit position, atoms before, width of the full atom, r5 or None, smallidx, run), smallidx and run being those in
    force for the group's small atoms.  Raises Refused for what is no valid frame — also for a stream that runs past
    its n_bytes into the padding, where the project's decoders, which know the padded length, only refuse what runs
    past the padding; no file here ends in between.  `mutant` plants one of MUTANTS."""
    assert mutant is None or mutant in MUTANTS
    h = parse_header(frame_bytes)
    natoms = h["natoms"]
    if natoms <= 9:
        return None, h["raw"], []
    sizes, bitsize, fields = field_widths(h["minint"], h["maxint"])
    width = bitsize or sum(fields)
    smallidx = h["smallidx"]
    if not FIRST_IDX <= smallidx < LAST_IDX:
        raise Refused("smallidx")
    cur = _Cursor(h["block"], h["n_bytes"])       # the stream is n_bytes long: the padding to a multiple of 4 is no part of it
    msb = mutant == "chunks msb first"
    out, trace, run = [], [], 0
    while len(out) < natoms:
        at = cur.pos
        if bitsize:
            full = cur.mixed(bitsize, sizes, msb)
        else:
            full = [cur.read(w) for w in fields]
        full = [c + m for c, m in zip(full, h["minint"])]
        r5, step = None, 0
        if cur.read(1):
            r5 = cur.read(5)
            step = r5 % 3 - 1
            run = r5 - r5 % 3
        elif mutant == "unflagged resets run":
            run = 0
        trace.append((at, len(out), width, r5, smallidx, run))
        if len(out) + 1 + run // 3 > natoms:
            raise Refused("a run passes the last atom")
        magic = MAGIC[smallidx]
        smallnum = (MAGIC[smallidx + step] if mutant == "smallnum after step" and FIRST_IDX <= smallidx + step < LAST_IDX
                    else magic) // 2
        prev = full
        for k in range(run // 3):
            d = cur.mixed(smallidx, [magic] * 3, msb)
            atom = [a + b - smallnum for a, b in zip(d, prev)]
            if k == 0 and mutant != "no swap":
                out += [atom, prev]          # the first small atom of a run is stored after the full atom, and precedes it
            elif k == 0:
                out += [prev, atom]
            else:
                out.append(atom)
            prev = atom
        if run == 0:
            out.append(full)
        smallidx += step
        if not FIRST_IDX <= smallidx < LAST_IDX:
            raise Refused("smallidx leaves the table")
    ints = np.array(out, dtype=np.int64).reshape(natoms, 3)
    return ints, to_f32(ints, h["precision"]), trace


def to_f32(ints, precision):
    """coordinate = int32 * (1 / precision), both in f32"""
    return ints.astype(np.int32).astype(np.float32) * (np.float32(1) / np.float32(precision))


def decode_file(buf, mutant=None):
    """every frame of a file -> list of (ints, xyz, trace, header)"""
    out, pos = [], 0
    while pos < len(buf):
        h = parse_header(buf, pos)
        out.append(reference_decode(buf[pos:h["end"]], mutant) + (h,))
        pos = h["end"]
    return out


def split_file(buf):
    """-> the frames' byte strings"""
    out, pos = [], 0
    while pos < len(buf):
        end = parse_header(buf, pos)["end"]
        out.append(buf[pos:end])
        pos = end
    return out


def small_extremes(f):
    """-> the smallidx values at which a file holds a small atom of (0, 0, 0), of (magic - 1,) * 3, of (magic / 2,) * 3"""
    zero, top, mid = set(), set(), set()
    for chosen, groups in zip(f.chosen, f.written):
        smallidx = chosen["smallidx"]
        for _, r5, smalls in groups:
            for d in smalls:
                m = MAGIC[smallidx]
                zero |= {smallidx} if d == [0, 0, 0] else set()
                top |= {smallidx} if d == [m - 1] * 3 else set()
                mid |= {smallidx} if d == [m // 2] * 3 else set()
            if r5 is not None:
                smallidx += r5 % 3 - 1
    return zero, top, mid


def reached(traces):
    """the states a list of traces visits -> dict of sets:
       widths       widths of full atoms
       r5           the five-bit fields read
       run3         small atoms per group, with or without a flag
       small        (smallidx, small atoms per group) of every group that has small atoms
       transitions  (small atoms per group before, after) at every flagged group
       stretches    (small atoms per group, length) of every maximal stretch of groups without a flag"""
    got = {k: set() for k in ("widths", "r5", "run3", "small", "transitions", "stretches")}
    for trace in traces:
        before, stretch = 0, 0
        for (_, _, width, r5, smallidx, run) in trace:
            got["widths"].add(width)
            got["run3"].add(run // 3)
            if run:
                got["small"].add((smallidx, run // 3))
            if r5 is None:
                stretch += 1
            else:
                if stretch:
                    got["stretches"].add((before, stretch))
                stretch = 0
                got["r5"].add(r5)
                got["transitions"].add((before, run // 3))
            before = run // 3
        if stretch:
            got["stretches"].add((before, stretch))
    return got


# ---- the builder -------------------------------------------------------------------------------------------------------
class _Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, nbits, v):
        assert 0 <= v < (1 << nbits), (nbits, v)
        self.acc = (self.acc << nbits) | v
        self.n += nbits
        while self.n >= 8:
            self.n -= 8
            self.out.append((self.acc >> self.n) & 0xff)
        self.acc &= (1 << self.n) - 1

    def mixed(self, nbits, sizes, nums):
        v = (nums[0] * sizes[1] + nums[1]) * sizes[2] + nums[2]
        assert v < (1 << nbits), (nbits, sizes, nums)
        while nbits > 8:
            self.put(8, v & 0xff)
            v >>= 8
            nbits -= 8
        self.put(nbits, v)

    def bytes(self):
        return bytes(self.out) + (bytes([(self.acc << (8 - self.n)) & 0xff]) if self.n else b"")


def expected_ints(minint, smallidx0, groups):
    """the coordinates that `groups` spell, atom by atom, in plain arithmetic (no bits) -> list of triples"""
    out, smallidx, run3 = [], smallidx0, 0
    for full, r5, smalls in groups:
        if r5 is not None:
            run3 = r5 // 3
        prev = [f + m for f, m in zip(full, minint)]
        half = MAGIC[smallidx] // 2 if 0 <= smallidx < LAST_IDX else 0
        chain = []
        for d in smalls:
            prev = [a + b - half for a, b in zip(d, prev)]
            chain.append(prev)
        first = [f + m for f, m in zip(full, minint)]
        out += chain[:1] + [first] + chain[1:]
        if r5 is not None:
            smallidx += r5 % 3 - 1
    return out


def build_frame(natoms, minint, maxint, smallidx0, groups, precision=1000.0, time=0.0, step=0, box=None, cut_bytes=None):
    """The bytes of one frame.  groups: list of (full triple, r5 or None, [small triples]) — the numbers as stored (a
    full atom's coordinate - minint, a small atom's offset + magic / 2) — written as given: neither the atom count nor
    the walk of smallidx is checked, only that every number fits its field and that every coordinate stays inside
    [minint, maxint].  cut_bytes: end the block after that many bytes."""
    sizes, bitsize, fields = field_widths(minint, maxint)
    for atom in expected_ints(minint, smallidx0, groups):
        assert all(a <= c <= b for a, c, b in zip(minint, atom, maxint)), (atom, minint, maxint)
    b, smallidx = _Bits(), smallidx0
    for full, r5, smalls in groups:
        assert all(0 <= f < s for f, s in zip(full, sizes)), (full, sizes)
        if bitsize:
            b.mixed(bitsize, sizes, full)
        else:
            for w, f in zip(fields, full):
                b.put(w, f)
        if r5 is None:
            b.put(1, 0)
        else:
            b.put(1, 1)
            b.put(5, r5)
        for d in smalls:
            assert all(0 <= x < MAGIC[smallidx] for x in d), (d, smallidx)
            b.mixed(smallidx, [MAGIC[smallidx]] * 3, d)
        if r5 is not None:
            smallidx += r5 % 3 - 1
    block = b.bytes()
    if cut_bytes is not None:
        block = block[:cut_bytes]
    box = np.eye(3, dtype=np.float32) * np.float32(10) if box is None else np.asarray(box, np.float32).reshape(3, 3)
    head = struct.pack(">iiif9fi", 1995, natoms, step, time, *[float(x) for x in box.reshape(9)], natoms)
    head += struct.pack(">f6iiI", precision, *minint, *maxint, smallidx0, len(block))
    return head + block + bytes(-len(block) % 4)


def build_file(frames):
    return b"".join(frames)


# ---- groups that visit what a script asks for ---------------------------------------------------------------------------
def _lcg(seed):
    x = (seed * 2654435761 + 12345) & 0xffffffffffffffff
    while True:
        x = (x * 6364136223846793005 + 1442695040888963407) & 0xffffffffffffffff
        yield x >> 20


def scripted_groups(natoms, minint, maxint, smallidx0, script, seed=0):
    """Groups for one frame of exactly natoms atoms.  script: r5 (int) or None per group; when it ends the frame is
    filled with groups without a flag, and closed with one flagged group whose run takes the atoms that are left.
    The values cycle through the edges — full atoms all 0, all size - 1, size - 1 in one dimension at a time, anything;
    small atoms 0, magic - 1, magic / 2 in all three, mixed, anything — bent only as far as the bounding box demands:
    per dimension the chain of offsets alternates between the two extremes, or stays put, where it would leave the box."""
    sizes, _, _ = field_widths(minint, maxint)
    rnd = _lcg(seed)
    groups, atoms, smallidx, run3, g = [], 0, smallidx0, 0, 0
    script = list(script)
    while atoms < natoms:
        left = natoms - atoms
        if g < len(script) and (script[g] is None or 1 + script[g] // 3 <= left) and \
                (script[g] is not None or 1 + run3 <= left):
            r5 = script[g]
        elif g >= len(script) and 1 + run3 <= left:
            r5 = None
        else:
            r5 = 3 * (left - 1) + 1        # the run that ends the frame (no step of smallidx)
        if r5 is not None:
            run3 = r5 // 3
        magic = MAGIC[smallidx]
        half = magic // 2
        kind = (g + seed) % 5
        smalls = []
        for k in range(run3):
            if kind == 0:
                d = [0, 0, 0]
            elif kind == 1:
                d = [magic - 1] * 3
            elif kind == 2:
                d = [half] * 3
            elif kind == 3:
                d = [[0, magic - 1, half][(k + c) % 3] for c in range(3)]
            else:
                d = [next(rnd) % magic for _ in range(3)]
            smalls.append(d)
        fkind = (g // 5 + g + seed) % 8
        full = [0, 0, 0]
        for c in range(3):
            want = [0, sizes[c] - 1, sizes[c] - 1 if c == 0 else 0, sizes[c] - 1 if c == 1 else 0,
                    sizes[c] - 1 if c == 2 else 0, next(rnd) % sizes[c], next(rnd) % sizes[c], next(rnd) % sizes[c]][fkind]
            for attempt in range(3):
                if attempt == 1:       # alternate between a value and its mirror image
                    for k in range(1, run3, 2):
                        smalls[k][c] = magic - 1 - smalls[k - 1][c]
                elif attempt == 2:     # stay put
                    for k in range(run3):
                        smalls[k][c] = half
                pos, lo, hi = 0, 0, 0
                for k in range(run3):
                    pos += smalls[k][c] - half
                    lo, hi = min(lo, pos), max(hi, pos)
                if hi - lo <= sizes[c] - 1:
                    break
            full[c] = min(max(want, -lo), sizes[c] - 1 - hi)
        groups.append((full, r5, smalls))
        atoms += 1 + run3
        if r5 is not None:
            smallidx += r5 % 3 - 1
        g += 1
    assert atoms == natoms
    return groups


def cube(width, skew=(7, -5, 0)):
    """three sizes (each <= 0xffffff) whose product has `width` bits"""
    s = int(round(2.0 ** ((width - 0.5) / 3.0)))
    sizes = [min(max(s + k, 1), 0xffffff) for k in skew]
    assert (sizes[0] * sizes[1] * sizes[2]).bit_length() == width, (width, sizes)
    return sizes


def box_of(sizes, low=None):
    """minint, maxint for the sizes"""
    low = [-(s // 3) for s in sizes] if low is None else low
    return list(low), [a + s - 1 for a, s in zip(low, sizes)]


class StreamFile:
    """one file of a family: frames (bytes each), the states it claims (see `reached`), groups to analyse, and per
    frame what the builder chose (for the packer's frame table)"""

    def __init__(self, name, claims=None):
        self.name, self.frames, self.claims, self.groups, self.chosen, self.expected = name, [], claims or {}, [], [], []
        self.natoms, self.written = None, []          # written: per frame the groups as build_frame got them

    def add(self, natoms, minint, maxint, smallidx0, groups, precision=1000.0, **kw):
        t = float(len(self.frames))
        self.frames.append(build_frame(natoms, minint, maxint, smallidx0, groups, precision, time=t, step=len(self.frames), **kw))
        sizes, bitsize, fields = field_widths(minint, maxint)
        self.chosen.append({"bitsize": bitsize, "bitsizeint": fields[0] | fields[1] << 8 | fields[2] << 16,
                            "sizeint": sizes, "smallidx": smallidx0, "minint": list(minint), "precision": precision})
        self.expected.append(expected_ints(minint, smallidx0, groups))
        self.written.append(groups)
        assert self.natoms in (None, natoms)
        self.natoms = natoms

    def scripted(self, natoms, minint, maxint, smallidx0, script, seed=0, precision=1000.0, **kw):
        self.add(natoms, minint, maxint, smallidx0, scripted_groups(natoms, minint, maxint, smallidx0, script, seed), precision, **kw)

    def data(self):
        return build_file(self.frames)

    def default_groups(self):
        n = self.natoms
        scattered = np.unique(np.array([(k * 37 + 11) % n for k in range(n // 5)], np.uint32))[::-1].copy()
        return [scattered, np.array([n - 1], np.uint32), np.array([0], np.uint32)] + self.groups


# runs of 0, 1, 2, 3, 4 and 8, steps both ways: smallidx stays within [start, start + 2] and ends where it started
MIXED_SCRIPT = [1, 5, None, 8, 25, None, None, 12, 3, 1, None, 10, 26, 24, None, 4, 14, 0, 10, 1]

VALUE_WIDTHS = (1, 8, 9, 31, 32, 33, 52, 53, 54, 56, 57, 63, 64, 65, 71, 72)


def sizes_for_width(width):
    return {1: [1, 1, 1], 8: [201, 1, 1], 9: [1, 1, 300], 53: [0xffffff, 0xffffff, 31], 72: [0xffffff] * 3}.get(width) or cube(width)


def family_values():
    """every width of a full atom at its edges, sizes of 1, three fields of 1, 26 and 32 bits; the atoms' values walk
    the corners of the bounding box (scripted_groups)"""
    n = 640
    narrow = StreamFile("values_narrow", {"widths": {w for w in VALUE_WIDTHS if w <= 53}, "run3": {0, 1, 2, 3, 4, 8}})
    wide = StreamFile("values_wide", {"widths": {w for w in VALUE_WIDTHS if w > 53}, "run3": {0, 1, 2, 3, 4, 8}})
    for k, w in enumerate(VALUE_WIDTHS):
        sizes = sizes_for_width(w)
        assert field_widths(*box_of(sizes))[1] == w
        lo, hi = box_of(sizes)
        (narrow if w <= 53 else wide).scripted(n, lo, hi, 9 + 4 * k, MIXED_SCRIPT * 6, seed=k, precision=[1000.0, 100.0, 12345.0][k % 3])
    for k, sizes in enumerate(([977, 1, 1], [1, 1, 977])):
        lo, hi = box_of(sizes, [5, -7, 3])
        narrow.scripted(n, lo, hi, 12, MIXED_SCRIPT * 6, seed=20 + k)
    fields = StreamFile("values_fields", {"widths": {1 + 26 + 32, 32 + 1 + 26, 26 + 32 + 1, 96}, "run3": {0, 1, 2, 3, 4, 8}})
    one, mid, top = (7, 7), (-2 ** 24, 2 ** 24 + 4), (INT_MIN, INT_MAX - 1)
    for k, dims in enumerate(([one, mid, top], [top, one, mid], [mid, top, one], [top, top, top])):
        lo, hi = [d[0] for d in dims], [d[1] for d in dims]
        assert sorted(field_widths(lo, hi)[2]) == ([32, 32, 32] if k == 3 else [1, 26, 32])
        fields.scripted(n, lo, hi, [30, 70, 9, 50][k], MIXED_SCRIPT * 6, seed=30 + k)
    return [narrow, wide, fields]


def _walk_script(phase):
    """smallidx 9 -> 72 -> 9, one step per group; runs cycle through 1, 2, 3 and 8"""
    runs = [1, 2, 3, 8]
    up = [3 * runs[(k + phase) % 4] + 2 for k in range(LAST_IDX - 1 - FIRST_IDX)]
    down = [3 * runs[(k + phase + 1) % 4] for k in range(LAST_IDX - 1 - FIRST_IDX)]
    return up + down


def family_small_widths():
    """small atoms of every width 9..72 under a full atom of at most 53 bits (two boxes), of 67 bits and of three fields
    (there wide enough in every dimension for 0 and magic - 1 in all three at once, up to the 72-bit joint maximum)"""
    out = []
    every = {(s, r) for s in range(FIRST_IDX, LAST_IDX) for r in (1, 2, 3, 8)}
    # "simple": two edges wide enough for the offsets of every smallidx (the hand-over above 53 bits sees large digits),
    # the third only 31 wide; "cube": three edges of about 185 000 steps, room for 0 and magic - 1 in all three at once
    # up to smallidx 55 — every width at which the simple loop divides a small atom in f64, magic[53]^3 - 1 included
    forms = {"simple": box_of([0xffffff, 0xffffff, 31]), "wide": box_of(cube(67)),
             "fields": ([-2 ** 25, INT_MIN, 0], [2 ** 25 + 4, INT_MAX - 1, 2 ** 27]),      # every edge beyond 2 magic[72]
             "cube": box_of(cube(53))}
    for name, (lo, hi) in forms.items():
        f = StreamFile("small_widths_" + name, {"small": every, "widths": {field_widths(lo, hi)[1] or sum(field_widths(lo, hi)[2])}})
        for phase in range(5):          # (the runs cycle with period 4, the values with period 5)
            f.scripted(700, lo, hi, FIRST_IDX, _walk_script(phase), seed=phase)
        out.append(f)
    assert field_widths(*forms["simple"])[1] == 53 and field_widths(*forms["wide"])[1] == 67
    assert field_widths(*forms["cube"])[1] == 53
    assert field_widths(*forms["fields"])[2] == [27, 32, 28]
    return out


def family_runs():
    """every r5, every transition between runs 0, 1, 2 and 8, stretches without a flag of 1, 2, 63, 64, 65 and 130
    groups with run 0 and with run 8"""
    out = []
    every_r5 = list(range(32))
    pairs = [3 * b + 1 for a in (0, 1, 2, 8) for b in (a, 0, a, 1, a, 2, a, 8)]
    trans = {(a, b) for a in (0, 1, 2, 8) for b in (0, 1, 2, 8)}
    for name, sizes in (("simple", cube(40)), ("wide", cube(60))):
        lo, hi = box_of(sizes)
        f = StreamFile("runs_" + name, {"r5": set(every_r5), "transitions": trans, "run3": set(range(11))})
        f.scripted(640, lo, hi, 20, every_r5 + every_r5[::-1], seed=1)
        f.scripted(640, lo, hi, 33, pairs, seed=2)
        out.append(f)
    lengths = (1, 2, 63, 64, 65, 130)
    # run 0: [flag, run 0] + L groups without one, then flagged groups
    lo, hi = box_of(cube(40))
    f = StreamFile("runs_stretch0", {"stretches": {(0, n) for n in lengths}})
    for k, n in enumerate(lengths):
        f.scripted(640, lo, hi, 15, [7, 1] + [None] * n + [4, 10, 1, 25] * 40, seed=k)
    out.append(f)
    # run 8 at smallidx 60: a group is 541 bits, 64 of them 4.3 KB — the scan's 8-KB window is reloaded inside the stretch
    lo, hi = box_of(cube(60))
    f = StreamFile("runs_stretch8", {"stretches": {(8, n) for n in lengths}})
    for k, n in enumerate(lengths):
        f.scripted(1200, lo, hi, 60, [1, 25] + [None] * n + [4, 10, 1, 25] * 40, seed=k)
    out.append(f)
    return out


def family_checkpoints():
    """group boundaries on every residue around the checkpoints at multiples of 256 atoms, groups of 11 atoms, and
    analysed groups that end on every kind of atom"""
    out = []
    lo, hi = box_of(cube(40))
    n = 800
    f = StreamFile("checkpoints_nine", {"run3": {0, 8}})
    for k in range(10):
        f.scripted(n, lo, hi, 25, [1] * k + [25] + [None] * 200, seed=k)             # one stretch without a flag
        f.scripted(n, lo, hi, 25, [1] * k + [25] * 200, seed=k + 10)                 # every group flagged
    out.append(f)
    f = StreamFile("checkpoints_eleven", {"run3": {0, 10}, "r5": {31}})
    for k in range(11):
        f.scripted(n, lo, hi, 30, [1] * k + [31] + ([None] * 200 if k % 2 else [31] * 200), seed=k)
    out.append(f)
    # one structure for every frame: singles, runs of 1, 2 and 8, a few times over (the groups come from its trace)
    f = StreamFile("checkpoints_ends", {"run3": {0, 1, 2, 8}})
    script = ([1, None, 4, None, 7, 25, None, 1] * 40)
    for k in range(3):
        f.scripted(n, lo, hi, 22, script, seed=k)
    trace = reference_decode(f.frames[0])[2]
    ends = {0, n - 1}
    seen = set()
    for (_, before, _, _, _, run) in trace:
        if run and (run // 3, before // 256) not in seen and run // 3 in (1, 2, 8):
            seen.add((run // 3, before // 256))
            ends |= {before, before + 1, before + run // 3}        # the swapped small atom, the full atom, the run's last
    ends |= set(range(256 - 9, 256 + 10)) | set(range(512 - 1, 512 + 9))
    for e in sorted(ends):
        few = sorted({(e * 7 + 3) % (e + 1), e // 2, e})
        f.groups.append(np.array(few[::-1], np.uint32))
    out.append(f)
    return out


def family_mixed_launch():
    """frames of the 53-bit 'simple' form, of 54..72 bits and of three fields in ONE launch"""
    forms = [box_of(cube(40)), box_of(cube(60)), box_of(cube(67)), ([-2 ** 24, 4, INT_MIN], [2 ** 24 + 4, 6, INT_MAX - 1]),
             box_of([977, 1, 1]), box_of([1, 1, 300]), box_of([1, 1, 1])]        # sizes of 1 through the general loop's divisions
    n = 640
    out = []
    box = np.eye(3) * 1e7         # (nm: wider than the 2^32 grid steps of the three-field frames, for runs through the analysis)
    f = StreamFile("mixed_alternating", {"widths": {40, 60, 67, 10, 9, 1}})
    for k, form in enumerate([0, 1, 2, 3, 4, 3, 2, 1, 0, 5, 0, 3, 1, 2, 0, 6, 0, 2, 0]):
        f.scripted(n, *forms[form], 9 + 3 * k, MIXED_SCRIPT * 6, seed=k, box=box)
    out.append(f)
    for name, usual, odd in (("mixed_one_wide", 0, 2), ("mixed_one_simple", 3, 0)):
        f = StreamFile(name)
        for k in range(65):
            f.scripted(n, *forms[odd if k == 37 else usual], 9 + k % 60, MIXED_SCRIPT * 6, seed=k, box=box)
        out.append(f)
    return out


def family_refused():
    """five frames each, the middle one no valid frame: a step to smallidx 8, to 73, a run past the last atom, a block
    that ends inside an atom -> list of StreamFile (frames 0, 1, 3, 4 valid)"""
    lo, hi = box_of(cube(40))
    n = 640
    out = []
    good = scripted_groups(n, lo, hi, 20, MIXED_SCRIPT * 6, seed=3)
    bad = {
        "refused_idx8": (9, scripted_groups(n, lo, hi, 9, [1] * 300, seed=1)[:300] + [([1, 2, 3], 0, [])] + [([1, 2, 3], None, [])] * 339),
        "refused_idx73": (72, scripted_groups(n, lo, hi, 72, [1] * 300, seed=1)[:300] + [([1, 2, 3], 2, [])] + [([1, 2, 3], None, [])] * 339),
        "refused_run": (20, scripted_groups(n, lo, hi, 20, [1] * 640, seed=1)[:636] + [([500, 500, 500], 3 * 4 + 1, [[50, 50, 50]] * 4)]),
    }
    for name, (idx, groups) in bad.items():
        f = StreamFile(name)
        for k in range(5):
            if k == 2:
                f.add(n, lo, hi, idx, groups)
            else:
                f.add(n, lo, hi, 20, good)
        out.append(f)
    f = StreamFile("refused_cut")
    for k in range(5):
        f.add(n, lo, hi, 20, good, **({"cut_bytes": 1001} if k == 2 else {}))
    out.append(f)
    return out


FAMILIES = {"values": family_values, "small_widths": family_small_widths, "runs": family_runs,
            "checkpoints": family_checkpoints, "mixed_launch": family_mixed_launch}
_cache = {}


def family(name):
    """the family's files, built once per process"""
    if name not in _cache:
        _cache[name] = (family_refused if name == "refused" else FAMILIES[name])()
    return _cache[name]


def all_files():
    return [f for name in FAMILIES for f in family(name)]


_refs = {}


def reference_of(f):
    """(ints [F, N, 3] int64, xyz [F, N, 3] float32, traces) of a StreamFile by the reference decoder, once per process"""
    if f.name not in _refs:
        dec = [reference_decode(fr) for fr in f.frames]
        _refs[f.name] = (np.stack([d[0] for d in dec]), np.stack([d[1] for d in dec]), [d[2] for d in dec])
    return _refs[f.name]


def write_files(directory, files):
    """-> {name: path}"""
    paths = {}
    for f in files:
        paths[f.name] = str(directory / (f.name + ".xtc"))
        with open(paths[f.name], "wb") as fp:
            fp.write(f.data())
    return paths


def same_bits(a, b, what=""):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32), err_msg=what)


def device_decode(engine, paths, group=None, chunk=64, **kw):
    """-> xyz [F, n_out, 3] decoded by the device from packed windows (the output is pre-filled with NaN: a slot that
    nothing wrote shows)"""
    import torch
    from gorder_amd import xtc
    out = []
    for w in xtc.pack_trajectory(paths, group=group, chunk=chunk, threads=2, **kw):
        n = len(w["time"])
        n_out = w["n_atoms_file"] if group is None else len(group)
        blob = torch.from_numpy(w["blob"]).cuda()
        frames = torch.from_numpy(w["frames"].view(np.uint8).reshape(-1).copy()).cuda()
        slot = None if w["slot_of"] is None else torch.from_numpy(w["slot_of"]).cuda()
        xyz = torch.full((n, n_out, 3), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        engine.xtc_decode(blob.data_ptr(), blob.numel(), frames.data_ptr(), n, w["n_atoms_file"],
                          0 if slot is None else slot.data_ptr(), w["n_stop"], xyz.data_ptr(), n_out)
        engine.synchronize()
        out.append(xyz.cpu().numpy())
    return np.concatenate(out) if out else np.zeros((0, 0, 3), np.float32)
