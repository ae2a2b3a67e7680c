"""Deterministic batches that put a carried key of the ORF stage's six scanned planes (kg_orfs.hpp) across every border at which
the prefix maximum hands its running value on, shared by tests/test_orf_scan_cases_host.py (layout arithmetic, the numpy models
and a broken-carry twin, no GPU) and tests/test_gpu_orf_scan_edges.py (the device against the models).  Imports nothing from
kmergutsjava_amd but the record dtypes.

The layout, restated from OrfPlanes::plan and orf_summary_kernel: rows(s) = ceil((L_s // 3) / T), tb = their prefix sum,
n_tiles = 3 tb[n_seqs]; the item of (s, g, t) in a front-to-back plane is 3 tb[s] + g rows(s) + t, in a mirrored plane
n_tiles - 1 - that.  orf_scan_apply_kernel hands the running maximum from a thread's 16 items to the next thread and from a
wave's 1024 to the next wave, orf_tile_max_kernel / build_tile_scan_kernel from a workgroup's 4096 to the next scan tile, and
build_tile_scan_kernel from 256 scan tiles to its next step.

A case is one batch: tiny filler contigs (3 to 8 bytes, one tile row, stops and starts of both strands), one poly-A target with
planted codons, and fillers behind it.  Everything below speaks of a plane in *plane order*: the order in which the plane is
stored and scanned, which for the three mirrored planes is the contigs, phases and tiles backwards.  `lead` fillers lie in
front of the target in plane order (behind it in the batch for a mirrored plane); the target has R tiles per phase; the wanted
codon lies in plane-order tile pa of plane-order phase gm, so its item is src = 3 lead + gm R + pa; the tiles pa + 1 .. pa + d
hold nothing wanted; the query lies in tile pa + d + 1 = R - 1, the last one, so the consumer walks inside that tile and then
reads item r = src + d.  The last tile is what lets one batch serve the region kernel (u, e, b, i*), the free enumerator (the
run that reaches the contig's end reads `outer` there, and a first run's start search ends or begins there) and the start
searches, whose other end is the contig's end.

Families (B a border, src < B <= r always):
  tight       src = B - 1, r = B
  far         src = B - 17, r = B + 16 (B = THREAD: there is no item -1, so src = 2 B - 17 = 15 and r = 2 B + 16 = 48: the key
              still passes a whole thread slice, items 16 .. 31, and two thread borders)
  superseded  as far, plus a second wanted codon in the tile at item B: the nearer one wins
  no_leak     the target's segment holds nothing wanted; the segment in front of it in plane order has a wanted codon in its
              last tile.  'phase': that segment is the neighbouring phase of the same contig and the target's segment begins at
              item B exactly.  'contig': it is the neighbouring contig's; a contig begins at a multiple of 3 and no border is
              one, so the target's segment begins at B - B % 3 and the query reads item B = its tile B % 3.
make(family, plane, B) -> Case; repair_case(family, clamp, strand, B) -> RepairCase."""
from typing import NamedTuple, Optional

import numpy as np

import orfs_model as O

T = 128                                                 # kOrfTile
THREAD, WAVE, TILE, STEP = 16, 1024, 4096, 256 * 4096
BORDERS = (THREAD, WAVE, TILE, 2 * TILE, STEP)
FAMILIES = ("tight", "far", "superseded", "no_leak_phase", "no_leak_contig")
FREE = 16
MIN_RES = 3                                             # no filler has three codons in a frame

DOWN_FSTOP, DOWN_RSTOP, DOWN_RSTART, UP_FSTOP, UP_FSTART, UP_RSTOP = range(6)
PLANE_NAMES = ("DownFStop", "DownRStop", "DownRStart", "UpFStop", "UpFStart", "UpRStop")
# strand of the consumer, the planted spelling on the forward bytes, what the region kernel asks the plane for
STRAND = (0, 1, 1, 0, 0, 1)
SPELL = (b"TAA", b"TTA", b"CAT", b"TAA", b"ATG", b"TTA")
ROLE = ("u", "e", "b", "e", "b", "u")
MIRRORED = (False, False, False, True, True, True)
HAS_FREE = (True, False, True, False, True, True)       # orf_free_kernel reads outer from 0 and 5, its start search 2 and 4
# the forward triplets of a plane's class, start planes by the bits of start_codons
_CLASS = (("TAA", "TAG", "TGA"), ("TTA", "CTA", "TCA"), ("CAT", "CAC", "CAA"), ("TAA", "TAG", "TGA"), ("ATG", "GTG", "TTG"),
          ("TTA", "CTA", "TCA"))

FILLERS = (b"TTATAA", b"TAA", b"CATTTAG", b"ATGTAGCA", b"TTA", b"CTATG", b"TCAT")
_FILLER_LENS = np.array([len(f) for f in FILLERS], dtype=np.int64)
OTHER_SIDE = 2                                          # fillers on the side that does not position the target


def start_codons_of(plane: int) -> int:
    return 7 if plane in (DOWN_RSTART, UP_FSTART) else 0


def fillers(n: int):
    """n fillers, cycling through FILLERS -> (bytes, lengths)"""
    k, rem = divmod(n, len(FILLERS))
    return b"".join(FILLERS) * k + b"".join(FILLERS[:rem]), np.concatenate([np.tile(_FILLER_LENS, k), _FILLER_LENS[:rem]])


class Case(NamedTuple):
    name: str
    family: str
    plane: int
    B: int
    g: int                  # forward phase of the target's segment
    src: int                # item the answer's key originates at (for superseded: the carried, losing one), in plane order
    r: int                  # item the consumer reads
    R: int                  # tile rows of the target
    t_src: Optional[int]    # forward tiles: the source, the superseding codon, the one read, the query's
    t_sup: Optional[int]
    t_read: int
    t_query: int
    found: Optional[int]    # forward codon m of phase g the read must answer with, None: nothing
    start_codons: int
    front: int              # fillers in front of the target in the batch, and behind it
    back: int
    near_front: bytes       # the neighbouring contig of no_leak_contig (b"": none), directly in front of / behind the target
    near_back: bytes
    target: bytes
    rows: tuple             # (strand, frame, j0, j1) of the regions, all on the target
    expect: tuple           # per region: dict(left, right, n_res, flags, start_codon, first_inner)
    free: Optional[dict]    # the free candidate of (target, strand, frame) that the read decides, None: the plane has no reader there

    @property
    def target_seq(self) -> int:
        return self.front + (1 if self.near_front else 0)

    def batch(self):
        """-> (bytes, offsets)"""
        fb, fl = fillers(self.front)
        bb, bl = fillers(self.back)
        mid = [x for x in (self.near_front, self.target, self.near_back) if x]
        lens = np.concatenate([fl, np.array([len(x) for x in mid], np.int64), bl])
        off = np.zeros(lens.size + 1, dtype=np.int64)
        np.cumsum(lens, out=off[1:])
        return fb + b"".join(mid) + bb, off

    def regions(self) -> np.ndarray:
        L = len(self.target)
        return O.regions_of([O.codon_region(L, strand, f, j0, j1, seq=self.target_seq) for strand, f, j0, j1 in self.rows])


def _place(S: int, d: int, prefer: int, min_pa: int = 0):
    """(gm, R, pa, lead) with 3 lead + gm R + pa == S and R == pa + d + 2, the phase `prefer` where the arithmetic allows it."""
    for gm in (prefer, (prefer + 2) % 3, (prefer + 1) % 3):
        for pa in range(min_pa, min_pa + 6):
            R = pa + d + 2
            rem = S - gm * R - pa
            if rem >= 0 and rem % 3 == 0:
                return gm, R, pa, rem // 3
    raise AssertionError("no layout puts the source at item %d" % S)


def _record(L, strand, f, n, b, e, flags, sc, inner):
    xs, xe = f + 3 * b, f + 3 * min(e, n - 1) + 2
    left, right = (xs, xe) if not strand else (L - 1 - xe, L - 1 - xs)
    return dict(left=left, right=right, n_res=min(e, n) - b, flags=flags, start_codon=sc, first_inner=inner)


def _src_r(family: str, B: int):
    if family == "tight":
        return B - 1, B
    return (B - 17, B + 16) if B > THREAD else (2 * B - 17, 2 * B + 16)


def make(family: str, plane: int, B: int) -> Case:
    idx = FAMILIES.index(family) + plane + BORDERS.index(B)
    mirrored, strand, spell, role = MIRRORED[plane], STRAND[plane], SPELL[plane], ROLE[plane]
    o_src, o_sup, qo, trim = (5, 64, 97, 13)[idx % 4], (70, 6, 33)[idx % 3], (7, 40, 21)[(idx // 2) % 3], idx % 3
    near, plants = b"", []
    if family.startswith("no_leak"):
        if family == "no_leak_phase":
            k, gm, R, lead = next((k, gm, k + 2, (B - k - gm * (k + 2)) // 3) for k in range(3) for gm in (1 + idx % 2, 2 - idx % 2)
                                  if B - k - gm * (k + 2) >= 0 and (B - k - gm * (k + 2)) % 3 == 0)
        else:
            k, gm = B % 3, 0
            R, lead = k + 2, (B - k) // 3 - 1           # the neighbouring contig is one of the (B - k) / 3 in front
            near = (spell * 2) if mirrored else b"AC" + spell * 2       # its phase next to the target reads the wanted codon twice
        src, r, pa, p_read, p_sup = B - k - 1, B, None, k, None
    else:
        src, r = _src_r(family, B)
        gm, R, pa, lead = _place(src, r - src, idx % 3)
        p_read, p_sup = pa + r - src, (pa + (B - src) if family == "superseded" else None)
    g = 2 - gm if mirrored else gm
    fwd = (lambda p: R - 1 - p) if mirrored else (lambda p: p)
    L = 3 * T * R - trim
    n = (L - g) // 3
    f = (L - g) % 3 if strand else g
    t_query = fwd(R - 1)
    m_src = m_sup = found = None
    if pa is not None:
        m_src = found = fwd(pa) * T + o_src
        plants.append((g, m_src))
        if p_sup is not None:
            m_sup = found = fwd(p_sup) * T + o_sup
            plants.append((g, m_sup))
    elif family == "no_leak_phase":
        g_prev = 2 - (gm - 1) if mirrored else gm - 1
        plants.append((g_prev, fwd(R - 1) * T + 5))     # the last tile, in plane order, of the segment in front
    body = bytearray(b"A" * L)
    for gp, m in plants:
        assert gp + 3 * m + 3 <= L
        body[gp + 3 * m:gp + 3 * m + 3] = spell
    j_of = (lambda m: n - 1 - m) if strand else (lambda m: m)
    jf = None if found is None else j_of(found)
    sc = start_codons_of(plane)
    P5, HS, INT = O.PARTIAL5, O.HAS_STOP, O.INTERRUPTED
    rows, expect = [], []
    if role == "u":
        # down: the last stop below the region, which begins qo + 1 codons into the query tile; up: mirrored
        m_a = t_query * T + qo + 1 if not mirrored else qo - 3
        ja, jb = sorted((j_of(m_a), j_of(m_a + 2)))
        rows.append((strand, f, ja, jb))
        b = 0 if jf is None else jf + 1
        expect.append(_record(L, strand, f, n, b, n, P5 if jf is None else 0, 0, -1))
        free = _record(L, strand, f, n, b, n, FREE | (P5 if jf is None else 0), 0, -1)
    elif role == "e":
        m_a = t_query * T + qo + 1 if not mirrored else qo - 3
        ja, jb = sorted((j_of(m_a), j_of(m_a + 2)))
        rows.append((strand, f, ja, jb))
        expect.append(_record(L, strand, f, n, 0, n if jf is None else jf, P5 | (0 if jf is None else HS), 0, -1))
        # i*: a region from the query tile over everything planted
        m_far = m_src if m_src is not None else fwd(0) * T + 5
        ja, jb = sorted((j_of(t_query * T + qo), j_of(m_far - 2 if not mirrored else m_far + 2)))
        rows.append((strand, f, ja, jb))
        expect.append(_record(L, strand, f, n, 0, n, P5 | (0 if jf is None else INT), 0, -1 if jf is None else jf))
        free = None
    else:
        # the first start of the frame, the region three codons behind everything planted
        m_far = m_src if m_src is not None else fwd(0) * T + 5
        m_a = m_far - 3 if not mirrored else m_far + 3
        ja, jb = sorted((j_of(m_a), j_of(m_a - 2 if not mirrored else m_a + 2)))
        rows.append((strand, f, ja, jb))
        b = 0 if jf is None else jf
        expect.append(_record(L, strand, f, n, b, n, P5, 0 if jf is None else 1, -1))
        free = _record(L, strand, f, n, b, n, FREE | P5, 0 if jf is None else 1, -1)
    if not HAS_FREE[plane]:
        free = None
    n_near = 1 if near else 0
    front, back = (OTHER_SIDE, lead) if mirrored else (lead, OTHER_SIDE)
    return Case(name="%s-%s-%d" % (family, PLANE_NAMES[plane], B), family=family, plane=plane, B=B, g=g, src=src, r=r, R=R,
                t_src=None if pa is None else fwd(pa), t_sup=None if p_sup is None else fwd(p_sup), t_read=fwd(p_read), t_query=t_query,
                found=found, start_codons=sc, front=front, back=back, near_front=b"" if mirrored else near,
                near_back=near if mirrored else b"", target=bytes(body), rows=tuple(rows), expect=tuple(expect), free=free)


ALL = [(family, plane, B) for family in FAMILIES for plane in range(6) for B in BORDERS]


# ---- the repair's two clamps ------------------------------------------------------------------------------------------------

REPAIR_FAMILIES = ("tight", "far", "superseded")
REPAIR_BORDERS = (WAVE, TILE)
# (clamp, strand) -> the plane the search reads: repair_stop_after is orf_find_up on '+' and orf_find_down on '-'
REPAIR_PLANE = {("after", 0): UP_FSTOP, ("after", 1): DOWN_RSTOP, ("before", 0): DOWN_FSTOP, ("before", 1): UP_RSTOP}
REPAIR_ALL = [(family, clamp, strand, B) for family in REPAIR_FAMILIES for clamp in ("after", "before") for strand in (0, 1)
              for B in REPAIR_BORDERS]


class RepairCase(NamedTuple):
    name: str
    family: str
    clamp: str              # 'after': a stop behind the first segment's evidence clamps J to hi; 'before': one in front of the
    strand: int             # second segment's clamps it to lo
    plane: int
    B: int
    g: int
    src: int
    r: int
    R: int
    t_src: int
    t_sup: Optional[int]
    t_read: int
    t_query: int
    found: int              # forward codon m of phase g
    front: int
    back: int
    text: bytes             # the target on its strand (repair_cases.lay lays it on either)
    calls: tuple            # (frame, first codon, last codon, count) on the strand
    pos: int                # the junction's pos as the record holds it
    merge_gap: int

    @property
    def target_seq(self) -> int:
        return self.front

    def items(self):
        """what the batch helper of tests/test_gpu_repair.py takes: (text, strand, calls on the strand) per contig"""
        cyc = len(FILLERS)
        return ([(FILLERS[i % cyc], 0, []) for i in range(self.front)] + [(self.text, self.strand, list(self.calls))] +
                [(FILLERS[i % cyc], 0, []) for i in range(self.back)])


def repair_case(family: str, clamp: str, strand: int, B: int) -> RepairCase:
    idx = REPAIR_FAMILIES.index(family) + (clamp == "before") + strand + REPAIR_BORDERS.index(B)
    plane = REPAIR_PLANE[(clamp, strand)]
    mirrored = MIRRORED[plane]
    o_src, o_sup, qo = (5, 64, 97, 13)[idx % 4], (70, 6, 33)[idx % 3], (7, 40, 21)[(idx // 2) % 3]
    src, r = _src_r(family, B)
    d = r - src
    gm, R, pa, lead = _place(src, d, idx % 3, min_pa=d + 3)    # room for the other segment twice as far away
    p_sup = pa + (B - src) if family == "superseded" else None
    g = 2 - gm if mirrored else gm
    fwd = (lambda p: R - 1 - p) if mirrored else (lambda p: p)
    L = 3 * T * R
    fr = (-g) % 3 if strand else g                              # the frame of the stop: g = (L - fr) % 3 on '-'
    n = (L - fr) // 3
    j_of = (lambda m: n - 1 - m) if strand else (lambda m: m)
    t_query = fwd(R - 1)
    m_src = fwd(pa) * T + o_src
    m_sup = None if p_sup is None else fwd(p_sup) * T + o_sup
    found = m_src if m_sup is None else m_sup
    jq = j_of(t_query * T + qo + 1 if not mirrored else qo - 1)                # lp ('after') or gq ('before')
    js, jf = j_of(m_src), j_of(found)
    text = bytearray(b"ATG" + b"GCA" * (L // 3 - 1))
    for m in (m_src, m_sup):
        if m is not None:
            x = fr + 3 * j_of(m)
            text[x:x + 3] = b"TAA"
    if clamp == "after":
        p, q = fr, (fr + 2) % 3
        lp, dist = jq, js - jq
        gq = lp + 2 * dist + 40
        J = p + 3 * jf
    else:
        q, p = fr, (fr + 1) % 3
        gq, dist = jq, jq - js
        lp = gq - 2 * dist - 40
        J = q + 3 * (jf + 1)
    assert dist > 0 and lp - 5 >= 1 and gq + 5 <= (L - q) // 3 - 1
    C, A = p + 3 * lp + 2, q + 3 * gq
    assert (C + 1 + A) // 2 > J if clamp == "after" else (C + 1 + A) // 2 < J
    front, back = (OTHER_SIDE, lead) if mirrored else (lead, OTHER_SIDE)
    return RepairCase(name="%s-%s-%s-%d" % (family, clamp, "-" if strand else "+", B), family=family, clamp=clamp, strand=strand, plane=plane,
                      B=B, g=g, src=src, r=r, R=R, t_src=fwd(pa), t_sup=None if p_sup is None else fwd(p_sup), t_read=fwd(pa + d),
                      t_query=t_query, found=found, front=front, back=back, text=bytes(text),
                      calls=((p, lp - 5, lp, 3), (q, gq, gq + 5, 3)), pos=J if not strand else L - 1 - J, merge_gap=A - C + 10)


# ---- the planes' keys in numpy ------------------------------------------------------------------------------------------------

def layout(off):
    """-> (rows, tb, n_tiles) of a batch"""
    lens = np.diff(np.asarray(off, dtype=np.int64))
    rows = (lens // 3 + T - 1) // T
    tb = np.zeros(rows.size + 1, dtype=np.int64)
    np.cumsum(rows, out=tb[1:])
    return rows, tb, int(3 * tb[-1])


def item_of(off, plane: int, s: int, g: int, t: int) -> int:
    """the item of tile t of phase g of contig s in the plane as it is stored"""
    rows, tb, n_tiles = layout(off)
    i = int(3 * tb[s] + g * rows[s] + t)
    return n_tiles - 1 - i if MIRRORED[plane] else i


def wanted_codons(contig: bytes, plane: int, g: int, start_codons: int) -> np.ndarray:
    """the forward codons m of phase g of a contig that have the plane's class"""
    names = [c for k, c in enumerate(_CLASS[plane]) if plane not in (DOWN_RSTART, UP_FSTART) or start_codons >> k & 1]
    n = (len(contig) - g) // 3 if len(contig) >= g else 0
    return np.array([m for m in range(n) if contig[g + 3 * m:g + 3 * m + 3].decode() in names], dtype=np.int64)


def plane_keys(seq, off, plane: int, start_codons: int) -> np.ndarray:
    """One plane's per-tile keys (segment << 31 | low 31 bits, as orf_summary_kernel writes them but for the sign bit) in the
    order the plane is stored, before the scan."""
    sb = np.frombuffer(seq, dtype=np.uint8) if not isinstance(seq, np.ndarray) else seq
    off = np.asarray(off, dtype=np.int64)
    n_seqs = off.size - 1
    lens = np.diff(off)
    rows, tb, n_tiles = layout(off)
    mirrored = MIRRORED[plane]
    # every item's segment
    s_item = np.repeat(np.arange(n_seqs, dtype=np.int64), 3 * rows)
    g_item = (np.arange(n_tiles, dtype=np.int64) - 3 * tb[s_item]) // np.maximum(rows[s_item], 1)
    seg = 3 * s_item + g_item
    low = np.zeros(n_tiles, dtype=np.int64)
    if sb.size >= 3:
        names = [c for k, c in enumerate(_CLASS[plane]) if plane not in (DOWN_RSTART, UP_FSTART) or start_codons >> k & 1]
        table = np.zeros(65, dtype=bool)
        for c in names:
            table["ACGT".index(c[0]) * 16 + "ACGT".index(c[1]) * 4 + "ACGT".index(c[2])] = True
        code = O._CODE[sb]
        c0, c1, c2 = code[:-2], code[1:-1], code[2:]
        idx = np.where((c0 < 4) & (c1 < 4) & (c2 < 4), c0 * 16 + c1 * 4 + c2, 64)
        x = np.arange(sb.size - 2, dtype=np.int64)
        s = np.repeat(np.arange(n_seqs, dtype=np.int64), lens)[:sb.size - 2]
        hit = np.flatnonzero(table[idx] & (x + 2 < off[s + 1]))
        s, rel = s[hit], x[hit] - off[s[hit]]
        g, m = rel % 3, rel // 3
        item = 3 * tb[s] + g * rows[s] + m // T
        np.maximum.at(low, item, (0x7FFFFFFF - m) if mirrored else m + 1)
    if mirrored:
        return (((3 * n_seqs - 1 - seg) << 31) | low)[::-1].copy()
    return (seg << 31) | low


def decode(key: int, plane: int, n_seqs: int, s: int, g: int):
    """What orf_find_up / orf_find_down make of a scanned key read for segment (s, g): the forward codon, None: nothing."""
    seg, low = int(key) >> 31, int(key) & 0x7FFFFFFF
    want = 3 * n_seqs - 1 - (3 * s + g) if MIRRORED[plane] else 3 * s + g
    if seg != want or low == 0:
        return None
    return 0x7FFFFFFF - low if MIRRORED[plane] else low - 1
