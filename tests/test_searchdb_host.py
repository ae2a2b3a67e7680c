"""The file form of a kg_searchdb without a GPU: tests/searchdb_model.py writes files from the header's statement of the format,
and kg_searchdb_open must name the first thing that is wrong with a bad one before it needs a device.  Also the new structures'
layout against gcc, and the bindings' view of the new calls."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

import cluster_model as M
import search_model as S
import searchdb_model as DM
import seed_model as SD
from kmergutsjava_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK = dict(window=12, trigger=563, extend=640)


def _targets(seed=5, n=7):
    rng = np.random.default_rng(seed)
    prots = [M.random_protein(rng, int(rng.integers(0, 60))) for _ in range(n)] + [b"QE" * 20 + M.random_protein(rng, 30)]
    return S.batch(prots + prots[-1:])                  # (the repeat and the copy: valid windows > pairs > k-mers)


@pytest.fixture(scope="module")
def good():
    seq, off = _targets()
    return DM.write(seq, off, names=b"t0\nt1\n")


def _open(tmp_path, data: bytes):
    """-> (return code, message) of kg_searchdb_open on a file of these bytes; a handle that opens is freed."""
    path = tmp_path / "db.kgsdb"
    path.write_bytes(data)
    lib = N.load()
    h = C.c_void_p()
    rc = lib.kg_searchdb_open(0, os.fsencode(str(path)), 0, C.byref(h))
    msg = lib.kg_last_error().decode() if rc else ""
    if rc == N.KG_OK:
        lib.kg_searchdb_free(h)
    return rc, msg


def _refresh(data: bytearray) -> bytes:
    """The header checksum recomputed: what a test changes behind it is then the first thing wrong."""
    struct.pack_into("<Q", data, DM.AT_CHECKSUM, DM.checksum(bytes(data[:DM.CHECKED])))
    return bytes(data)


def _bad(tmp_path, data, words):
    rc, msg = _open(tmp_path, data)
    assert rc == N.KG_ERR_FORMAT and msg.startswith(words), (rc, msg)


# ---- the model itself ---------------------------------------------------------------------------------------------------------------

def test_the_checksum_catches_every_single_changed_byte_and_the_length():
    rng = np.random.default_rng(1)
    data = bytearray(rng.integers(0, 256, size=203, dtype=np.uint8).tobytes())
    want = DM.checksum(bytes(data))
    assert DM.checksum(b"") == 0 and DM.checksum(b"\1") == 2 and DM.checksum(bytes(8) + b"\1") == 3 + 9
    for at in range(len(data)):
        for delta in (1, 0x80, 0xFF):
            changed = bytearray(data)
            changed[at] ^= delta
            assert DM.checksum(bytes(changed)) != want
    assert DM.checksum(bytes(data) + b"\0") != want


def test_the_model_reads_what_it_writes_with_seeds_and_a_mask():
    seq, off = _targets()
    for seed, mask in ((None, None), (SD.EXACT, None), (None, MASK), (SD.random_seed(np.random.default_rng(3), n_shapes=2, max_span=12), MASK)):
        data = DM.write(seq, off, seed=seed, mask=mask, names=b"names")
        got = DM.read(data)
        assert len(data) % 64 == 0 and got["has_seeds"] == (seed is not None) and got["has_mask"] == (mask is not None)
        assert got["sections"]["residues"] == bytes(seq) and got["sections"]["names"] == b"names"
        pk = np.frombuffer(got["sections"]["pairs"], dtype="<u8")
        starts = np.frombuffer(got["sections"]["run_starts"], dtype="<u4")
        assert (np.diff(pk.astype(np.int64)) > 0).all() and starts[0] == 0 and starts[-1] == pk.size == got["counts"]["pairs"]
        assert got["counts"]["valid_windows"] >= pk.size and (np.diff(starts.astype(np.int64)) > 0).all()
    plain, masked = DM.read(DM.write(seq, off))["counts"], DM.read(DM.write(seq, off, mask=MASK))["counts"]
    assert masked["valid_windows"] < plain["valid_windows"]          # the planted repeat is masked


# ---- kg_searchdb_open on bad files --------------------------------------------------------------------------------------------------

def test_a_good_file_gets_past_the_checks(tmp_path, good):
    rc, msg = _open(tmp_path, good)
    if torch.cuda.is_available():
        assert rc == N.KG_OK, msg
    else:
        assert rc == N.KG_ERR_DEVICE and msg.startswith("no HIP device"), (rc, msg)


def test_magic_version_and_length(tmp_path, good):
    _bad(tmp_path, b"XGSRCHDB" + good[8:], "wrong magic")
    data = bytearray(good)
    struct.pack_into("<I", data, 8, 2)
    _bad(tmp_path, _refresh(data), "wrong version: 2")
    data = bytearray(good)
    struct.pack_into("<I", data, 12, 512)
    _bad(tmp_path, _refresh(data), "wrong header bytes: 512")
    _bad(tmp_path, good[:-1], "the file has %d bytes, the header gives %d" % (len(good) - 1, len(good)))
    _bad(tmp_path, good + b"\0", "the file has %d bytes, the header gives %d" % (len(good) + 1, len(good)))
    _bad(tmp_path, good[:100], "the file has 100 bytes, fewer than the header's 448")
    rc, msg = _open(tmp_path, b"")
    assert rc == N.KG_ERR_FORMAT
    lib, h = N.load(), C.c_void_p()
    assert lib.kg_searchdb_open(0, os.fsencode(str(tmp_path / "none")), 0, C.byref(h)) == N.KG_ERR_IO
    assert lib.kg_last_error().decode().startswith("cannot open ")


def test_a_changed_header_byte_without_a_new_checksum(tmp_path, good):
    data = bytearray(good)
    data[16] ^= 1
    _bad(tmp_path, bytes(data), "header checksum mismatch")
    data = bytearray(good)
    data[400] = 1
    _bad(tmp_path, bytes(data), "header byte 400 is not 0")


@pytest.mark.parametrize("k,name", list(enumerate(DM.COUNTS)))
@pytest.mark.parametrize("delta", [-1, 1])
def test_each_header_count_off_by_one(tmp_path, good, k, name, delta):
    data = bytearray(good)
    value = struct.unpack_from("<q", data, 16 + 8 * k)[0] + delta
    struct.pack_into("<q", data, 16 + 8 * k, value)
    _bad(tmp_path, bytes(data), "header checksum mismatch")
    # with the header checksum made right again the count disagrees with its section.  valid_windows is a statistic that no
    # section's size follows from: the header checksum is all that guards it, and its range (the next test).
    want = {"n_db": "section offsets: ", "residues": "section residues: ", "pairs": "section pairs: ", "kmers": "section run starts: ",
            "names_bytes": "section names: "}
    if name != "valid_windows":
        _bad(tmp_path, _refresh(data), want[name])


def test_valid_windows_out_of_its_range(tmp_path, good):
    data = bytearray(good)
    pairs = struct.unpack_from("<q", data, 32)[0]
    struct.pack_into("<q", data, 48, pairs - 1)
    _bad(tmp_path, _refresh(data), "pairs out of range")
    struct.pack_into("<q", data, 48, -1)
    _bad(tmp_path, _refresh(data), "valid windows out of range")


def _with_offsets(good, change):
    """The file with its offsets section changed by change(int64 array) and that section's checksum made right again."""
    data = bytearray(good)
    at, n, _ = struct.unpack_from("<QQQ", data, DM.AT_SECTIONS)
    off = np.frombuffer(bytes(data[at:at + n]), dtype="<i8").copy()
    change(off)
    data[at:at + n] = off.tobytes()
    struct.pack_into("<Q", data, DM.AT_SECTIONS + 16, DM.checksum(off.tobytes()))
    return _refresh(data)


def test_offsets_that_decrease_are_too_long_or_do_not_end_at_the_residues(tmp_path, good):
    def decrease(off):
        off[3] = off[2] - 1
    _bad(tmp_path, _with_offsets(good, decrease), "protein 2: offsets decrease")

    def long(off):
        off[2:] += 1 << 24
    _bad(tmp_path, _with_offsets(good, long), "protein 1: 2^24 or more characters")

    def first(off):
        off[0] = 1
    _bad(tmp_path, _with_offsets(good, first), "offsets[0] is not 0")

    def last(off):
        off[-1] += 1
    _bad(tmp_path, _with_offsets(good, last), "the last offset is not the residue count")


@pytest.mark.parametrize("k,name", list(enumerate(DM.SECTIONS)))
def test_one_flipped_byte_in_each_section_and_in_its_padding(tmp_path, good, k, name):
    at, n, _ = struct.unpack_from("<QQQ", good, DM.AT_SECTIONS + 24 * k)
    words = {"run_starts": "run starts"}.get(name, name)
    for where in (at, at + n // 2, at + n - 1):
        data = bytearray(good)
        data[where] ^= 0x10
        _bad(tmp_path, bytes(data), "section %s: checksum mismatch" % words)
    if (at + n) % 64:
        data = bytearray(good)
        data[at + n] = 1
        _bad(tmp_path, bytes(data), "padding behind section %s is not 0" % words)


def test_bad_parameters_in_the_header(tmp_path):
    seq, off = _targets()
    data = bytearray(DM.write(seq, off, seed=SD.EXACT, mask=MASK))
    struct.pack_into("<i", data, DM.AT_MASK, 3)                     # window 3
    _bad(tmp_path, _refresh(data), "the header's parameters: window must be in 4..32")
    data = bytearray(DM.write(seq, off, seed=SD.EXACT))
    struct.pack_into("<i", data, DM.AT_SEEDS, 5)                    # n_shapes 5
    _bad(tmp_path, _refresh(data), "the header's parameters: n_shapes must be in 1..4")


# ---- the ABI and the bindings -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cname,cls", [("kg_searchdb_desc", "KgSearchDbDesc"), ("kg_search_db_stats", "KgSearchDbStats")])
def test_the_new_structures_sit_where_gcc_puts_them(tmp_path, cname, cls):
    struct_ = getattr(N, cls)
    fields = [f for f, _ in struct_._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kmerguts_hip.h"\nint main(void){\n' +
                   'printf("%%zu\\n", sizeof(%s));\n' % cname +
                   "".join('printf("%%zu\\n", offsetof(%s, %s));\n' % (cname, f) for f in fields) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == C.sizeof(struct_) == {"kg_searchdb_desc": 240, "kg_search_db_stats": 24}[cname]
    assert out[1:] == [getattr(struct_, f).offset for f in fields]


def test_the_header_s_constants_and_symbols():
    hdr = open(os.path.join(ROOT, "include", "kmerguts_hip.h")).read()
    assert "#define KG_SEARCHDB_VERSION %d\n" % DM.VERSION in hdr and "#define KG_SEARCHDB_HEADER_BYTES %d\n" % DM.HEADER_BYTES in hdr
    assert (N.SEARCHDB_VERSION, N.SEARCHDB_HEADER_BYTES) == (DM.VERSION, DM.HEADER_BYTES)
    lib = N.load()
    new = [n for n in N.EXPORTS if n.startswith("kg_searchdb_")] + ["kg_hitset_db_stats"]
    assert len(new) == 12 and all(hasattr(lib, n) for n in new)


def test_arguments_are_checked_before_the_device():
    lib, h = N.load(), C.c_void_p()
    off = np.array([0, 5, 3], dtype=np.int64)
    seq = np.zeros(8, dtype=np.uint8)
    rc = lib.kg_searchdb_build(0, seq.ctypes.data, off.ctypes.data, 2, None, None, None, 0, 0, 0, C.byref(h))
    assert rc == N.KG_ERR_ARG and lib.kg_last_error().decode().startswith("protein 1: offsets decrease")
    rc = lib.kg_searchdb_build(0, seq.ctypes.data, off.ctypes.data, 1, None, None, None, 0, 0, -1, C.byref(h))
    assert rc == N.KG_ERR_ARG and lib.kg_last_error().decode() == "query_room must be >= 0"
    rc = lib.kg_searchdb_build(0, seq.ctypes.data, off.ctypes.data, 1, None, None, None, 3, 0, 0, C.byref(h))
    assert rc == N.KG_ERR_ARG and lib.kg_last_error().decode() == "null names"
    st = N.KgSearchDbStats()
    assert lib.kg_hitset_db_stats(None, C.byref(st)) == N.KG_ERR_ARG
    assert lib.kg_searchdb_search(None, None, None, None, None, 0, 0, 0, 0, 0, None, None, None, C.byref(h)) == N.KG_ERR_ARG
    assert lib.kg_last_error().decode() == "null kg_searchdb"


# ---- the front ends, with the model in the device's place -------------------------------------------------------------------------------

import band_model as B  # noqa: E402
import ungapped_model as UM  # noqa: E402
from kmergutsjava_amd import make_search_db as MD  # noqa: E402
from kmergutsjava_amd import search_proteins as SP  # noqa: E402


def _fasta(ids, prots) -> bytes:
    return b"".join(b">" + i + b"\n" + p + b"\n" for i, p in zip(ids, prots))


def _model_search(seq, offsets, n_db, ungapped=None, band=None, min_shared=2, max_cand=8, max_db_per_kmer=256, align=None, device=0,
                  paths=None, ops=None, **kw):
    """hotpath.search_proteins' shape from band_model (tests/test_band_host.py has the same): needs ungapped and band."""
    hits, start, ung, counts, ucounts, bcounts = B.search_model(seq, offsets, n_db, band, min_ungapped=ungapped["min_score"],
                                                                min_shared=min_shared, max_cand=max_cand)
    st = dict(counts, ungapped=dict(ucounts, ms_ungapped=0.5), band=bcounts, ms_total=1.0)
    if paths is None:
        return hits, start, st, ung
    pth, starts, opsv = B.search_ops_model(seq, offsets, n_db, band, hits, ung, ops or "m", paths)
    st.update(traced=int((pth["status"] == N.PATH_TRACED).sum()), untraced=0)
    return (hits, start, pth, st) + ((starts, opsv) if ops else ()) + (ung,)


class _ModelDb:
    """hotpath.SearchDb's face over a model-written file: search() is the model's one-batch call on "targets, then queries"."""

    def __init__(self, path, room=1 << 20, device=0):
        self.file = DM.read(open(path, "rb").read())
        self.off = np.frombuffer(self.file["sections"]["offsets"], dtype="<i8").astype(np.int64)
        self.seq = self.file["sections"]["residues"]
        self.room, self.batches, self.closed = room, [], False

    def info(self):
        return dict(targets=self.off.size - 1, query_room=self.room, seeds=None, mask=None, mask_stats=None)

    def names(self):
        return self.file["sections"]["names"]

    def targets(self):
        return np.frombuffer(self.seq, dtype=np.uint8), self.off

    def reserve(self, n):
        self.room = max(self.room, n)

    def search(self, qseq, qoff, **kw):
        qoff = np.asarray(qoff, dtype=np.int64)
        assert int(qoff[-1]) <= self.room
        self.batches.append(qoff.size - 1)
        return _model_search(self.seq + bytes(qseq), np.concatenate([self.off, qoff[1:] + self.off[-1]]), self.off.size - 1, **kw)

    def close(self):
        self.closed = True

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


@pytest.fixture(scope="module")
def front(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("front")
    prots, n_db = B.indel_search(11, n_targets=6, n_related=5, length=80)
    ids = [b"p%d" % k for k in range(len(prots))]
    (tmp / "db.faa").write_bytes(_fasta(ids[:n_db], prots[:n_db]))
    (tmp / "q.faa").write_bytes(_fasta(ids[n_db:], prots[n_db:]))
    (tmp / "ann.tsv").write_bytes(b"".join(b"%s\tfunction %d\n" % (ids[k], k % 3) for k in range(n_db) if k != 2))
    functions = {ids[k]: (b"function %d" % (k % 3), None) for k in range(n_db) if k != 2}
    seq, off = S.batch(prots[:n_db])
    (tmp / "plain.kgsdb").write_bytes(DM.write(seq, off, names=MD.pack_names(ids[:n_db])))
    (tmp / "named.kgsdb").write_bytes(DM.write(seq, off, names=MD.pack_names(ids[:n_db], functions)))
    return tmp, prots, n_db


def _run(tmp, tag, **kw):
    out = {k: str(tmp / ("%s.%s" % (tag, k))) for k in ("o", "transfer", "alignments")}
    line = SP.search_proteins(kw.pop("database", []), [str(tmp / "q.faa")], out["o"], write_all=True, transfer=out["transfer"],
                              alignments=out["alignments"], ungapped=dict(min_score=0), band=4, paths="all", cigar="m", **kw)
    return line, tuple(open(out[k], "rb").read() for k in ("o", "transfer", "alignments"))


def test_an_index_in_the_database_s_place_gives_the_same_files_wherever_the_batches_are_cut(front):
    tmp, prots, n_db = front
    n_q = len(prots) - n_db
    line, want = _run(tmp, "d", database=[str(tmp / "db.faa")], annotations=str(tmp / "ann.tsv"), search=_model_search)
    assert all(want) and ", db:" not in line
    lens = [len(p) for p in prots[n_db:]]
    for batch, n_batches in ((None, 1), (1, n_q), (max(lens), None), (sum(lens[:2]), None), (sum(lens), 1)):
        opened = []

        def open_db(path, device=0):
            opened.append(_ModelDb(path))
            return opened[-1]

        got_line, got = _run(tmp, "db", db=str(tmp / "named.kgsdb"), batch_residues=batch, open_db=open_db)
        assert got == want, batch
        assert opened[0].closed and sum(opened[0].batches) == n_q and all(opened[0].batches)
        assert n_batches is None or len(opened[0].batches) == n_batches
        times = re.compile(r"\d+\.\d+")                                       # (the times add up over the batches)
        assert times.sub("#", got_line) == times.sub("#", line) + ", db: index (%d targets)" % n_db     # the counts are the one call's
    # -A beside an index without functions; an index without functions and no -A
    _, got = _run(tmp, "db", db=str(tmp / "plain.kgsdb"), annotations=str(tmp / "ann.tsv"), open_db=lambda p, device=0: _ModelDb(p), batch_residues=200)
    assert got == want
    with pytest.raises(ValueError, match="--transfer and --truth need -A, or an index made with make_search_db -A"):
        _run(tmp, "db", db=str(tmp / "plain.kgsdb"), open_db=lambda p, device=0: _ModelDb(p))


def test_a_query_longer_than_the_room_grows_it_and_no_queries_are_one_empty_batch(front, tmp_path):
    tmp, prots, n_db = front
    db = _ModelDb(str(tmp / "named.kgsdb"), room=10)
    _, want = _run(tmp, "d", database=[str(tmp / "db.faa")], annotations=str(tmp / "ann.tsv"), search=_model_search)
    _, got = _run(tmp, "db", db="x", open_db=lambda p, device=0: db)
    assert got == want and db.room == max(len(p) for p in prots[n_db:]) and db.batches == [1] * (len(prots) - n_db)
    assert SP.batch_cuts([], 5) == [0, 0] and SP.batch_cuts([3, 3, 3], 6) == [0, 2, 3] and SP.batch_cuts([9, 1, 1], 2) == [0, 1, 3]
    assert SP.batch_cuts([1, 1, 1], 1) == [0, 1, 2, 3] and SP.batch_cuts([2, 2], 100) == [0, 2]


def test_every_flag_that_conflicts_with_an_index_is_named(front, capsys):
    tmp, _, _ = front
    base = ["-q", str(tmp / "q.faa"), "-o", str(tmp / "h.tsv")]
    cases = [(["--db", "x", "-d", str(tmp / "db.faa")], "give -d or --db, not both"),
             ([], "one of -d and --db is required"),
             (["-d", str(tmp / "db.faa"), "--batch-residues", "5"], "--batch-residues needs --db"),
             (["--db", "x", "--batch-residues", "0"], "--batch-residues must be >= 1"),
             (["--db", "x", "--seeds", "reduced"], "--seeds beside --db: the seeds are the index's"),
             (["--db", "x", "--alphabet", "identity"], "--alphabet beside --db: the seeds are the index's"),
             (["--db", "x", "--shape", "11111111"], "--shape beside --db: the seeds are the index's"),
             (["--db", "x", "--mask"], "--mask both beside --db: the targets' mask is the index's"),
             (["--db", "x", "--mask", "targets"], "--mask targets beside --db: the targets' mask is the index's")]
    for flags, words in cases:
        with pytest.raises(SystemExit):
            SP.main(base + flags)
        assert words in capsys.readouterr().err, flags
    for kw, words in ((dict(database=["a"], db="x"), "give -d or --db, not both"), (dict(db="x", seeds="reduced"), "--seeds beside --db"),
                      (dict(db="x", mask=dict(sides="both")), "--mask both beside --db"), (dict(batch_residues=4), "--batch-residues needs --db")):
        with pytest.raises(ValueError, match=words):
            SP.search_proteins(kw.pop("database", []), [str(tmp / "q.faa")], str(tmp / "h.tsv"), **kw)
    # --mask queries is allowed beside --db and reaches the index's search as the queries' mask
    seen = {}

    class Db(_ModelDb):
        def search(self, qseq, qoff, mask=None, **kw):
            seen["mask"] = mask
            got = super().search(qseq, qoff, **kw)
            next(x for x in got if isinstance(x, dict))["mask"] = dict(masked_residues=3)
            return got

    line = SP.search_proteins([], [str(tmp / "q.faa")], str(tmp / "h.tsv"), db=str(tmp / "named.kgsdb"), open_db=lambda p, device=0: Db(p),
                       mask=dict(window=10, trigger=500, extend=600, sides="queries"), ungapped=dict(min_score=0), band=4,
                       batch_residues=150)
    assert seen["mask"] == dict(window=10, trigger=500, extend=600) and ", mask: 10/500/600 queries, masked residues: " in line


def test_the_names_blob_round_trips_and_make_search_db_writes_it(front, tmp_path):
    tmp, prots, n_db = front
    ids = [b"p%d" % k for k in range(n_db)]
    functions = {ids[0]: (b"alpha", b"otu"), ids[3]: (b"beta gamma", None)}
    assert MD.unpack_names(MD.pack_names(ids), n_db) == (ids, None)
    assert MD.unpack_names(MD.pack_names(ids, functions), n_db) == (ids, {ids[0]: (b"alpha", None), ids[3]: (b"beta gamma", None)})
    assert MD.unpack_names(MD.pack_names([]), 0) == ([], None) and MD.unpack_names(MD.pack_names([], {}), 0) == ([], {})
    assert MD.unpack_names(MD.pack_names([b"only"], {}), 1) == ([b"only"], {})
    with pytest.raises(MD.InputError):
        MD.unpack_names(MD.pack_names(ids), n_db + 1)
    seen = {}

    class Built:
        def save(self, path):
            seq, off = S.batch(prots[:n_db])
            open(path, "wb").write(DM.write(seq, off, names=seen["names"]))

        def info(self):
            return dict(targets=n_db, residues=1, valid_windows=2, pairs=3, kmers=4, device_bytes=5, seeds=None, mask=None, mask_stats=None)

        def close(self):
            seen["closed"] = True

    def build(seq, offsets, **kw):
        seen.update(kw, seq=seq, offsets=offsets)
        return Built()

    out = tmp_path / "made.kgsdb"
    line = MD.make_search_db([str(tmp / "db.faa")], str(out), annotations=str(tmp / "ann.tsv"), build=build)
    assert line.startswith("Targets: %d, residues: 1, " % n_db) and line.endswith(", functions: %d" % (n_db - 1)) and seen["closed"]
    assert seen["seq"] == b"".join(prots[:n_db]) and seen["seeds"] is None and seen["mask"] is None
    assert out.read_bytes() == (tmp / "named.kgsdb").read_bytes()
    got_ids, got_fn = MD.unpack_names(DM.read(out.read_bytes())["sections"]["names"], n_db)
    assert got_ids == ids and sorted(got_fn) == [i for i in ids if i != b"p2"]
    # the command line: the seed and mask flags reach the build
    got = {}
    import unittest.mock as mock
    with mock.patch.object(MD, "make_search_db", lambda *a, **kw: got.update(kw) or "ok"):
        assert MD.main(["-d", str(tmp / "db.faa"), "-o", str(out), "--seeds", "reduced", "--mask", "--mask-window", "10", "-A", "a.tsv"]) == 0
    assert got["seeds"] == dict(SP_SEEDS.BUILTIN["reduced"]) and got["mask"] == dict(window=10, trigger=563, extend=640) and got["annotations"] == "a.tsv"
    assert MD.seeds_of(None) is None
    for name in ("exact", "reduced"):                                           # what info() holds of a seed set describes that set
        cls, n_cls, masks = SP_SEEDS.resolve(dict(SP_SEEDS.BUILTIN[name]))[:3]
        back = MD.seeds_of(dict(n_shapes=len(masks), alphabet_size=n_cls, cls=list(cls), shape=list(masks)))
        assert SP_SEEDS.resolve(back)[:3] == (cls, n_cls, masks)


from kmergutsjava_amd import seeds as SP_SEEDS  # noqa: E402
