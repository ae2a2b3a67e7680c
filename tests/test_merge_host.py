"""The merge rule (include/kmerguts_hip.h, kg_table_merge_signatures) on the CPU: the two forms of tests/merge_model.py against each
other, answers worked out by hand, the union of the name indices, the layouts of the new structures, and the front end's files
with the device calls replaced by the model and synth.build_table."""
import ctypes as C
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import merge_model as M  # noqa: E402
import test_regions_host as H  # noqa: E402

from kmergutsjava_amd import _native as N  # noqa: E402
from kmergutsjava_amd import merge_tables as MT  # noqa: E402
from kmergutsjava_amd import synth  # noqa: E402
from kmergutsjava_amd.make_signatures import signature_text  # noqa: E402
from kmergutsjava_amd.make_table import parse_signatures  # noqa: E402

ROOT = os.path.dirname(HERE)
EMPTY = synth.EMPTY_KEY


def _both(base, new, fn_map=None, otu_map=None, policy="keep"):
    """merge_numpy == merge_dicts, the error included -> (U, counts) or the MergeError"""
    got = []
    for f in (M.merge_numpy, M.merge_dicts):
        try:
            U, c = f(base, new, fn_map, otu_map, policy)
            got.append((U.tobytes(), c))
        except M.MergeError as e:
            got.append((e.kind, e.value))
    assert got[0] == got[1], got
    if isinstance(got[0][0], str):
        return M.MergeError(*got[0])
    return np.frombuffer(got[0][0], dtype=N.SIGNATURE_DTYPE), got[0][1]


@pytest.mark.parametrize("seed", range(300))
def test_the_two_forms_agree(seed):
    """tiny random inputs: every policy, with and without maps, junk records (negative, 20^8, empty) among the base, streams cut
    short, and now and then an input that is an error (a k-mer twice, an index outside its map, a k-mer outside the range)"""
    rng = np.random.default_rng(seed)
    universe = rng.choice(M.MAX, size=int(rng.integers(1, 24)), replace=False)
    slots = int(rng.integers(0, 20))
    base = M.random_stream(rng, int(rng.integers(0, 12)), universe, slots)
    base = base[:int(rng.integers(0, slots + 1))] if seed % 3 == 0 else base          # a stream shorter than the header says
    new = M.random_sigs(rng, int(rng.integers(0, 12)), universe)
    fn_map = rng.integers(0, 3, 4).astype(np.int32) if seed % 2 else None
    otu_map = rng.integers(-2, 9, 3).astype(np.int32) if seed % 4 >= 2 else None
    if seed % 7 == 0 and len(new) > 1:
        new["kmer"][rng.integers(len(new))] = new["kmer"][0]                          # (may hit index 0 itself: then no error)
    if seed % 11 == 0 and len(base) > 1:
        base[rng.integers(len(base))] = base[0]
    if seed % 13 == 0 and len(new):
        new["functionIndex"][rng.integers(len(new))] = rng.choice([-1, 4])
    if seed % 17 == 0 and len(new):
        new["otuIndex"][rng.integers(len(new))] = 3
    if seed % 19 == 0 and len(new):
        new["kmer"][rng.integers(len(new))] = rng.choice([-1, M.MAX])
    for policy in M.POLICIES:
        r = _both(base, new, fn_map, otu_map, policy)
        if not isinstance(r, M.MergeError):
            U, c = r
            assert (np.diff(U["kmer"]) > 0).all() and c["merged"] == c["base"] + c["added"] - c["dropped"]
            assert c["added"] + c["conflicts"] == c["added_in"] and c["conflicts_same_function"] <= c["conflicts"] <= c["base"]


# ---- answers worked out by hand -----------------------------------------------------------------------------------------------

BASE = M.sigs([(EMPTY, 0, 0, 0, 0), (40, 1, 10, 5, 0.5), (-3, 9, 9, 9, 9), (7, 2, 20, 6, 1.0), (M.MAX, 0, 0, 0, 0), (EMPTY + 1, 0, 0, 0, 0),
               (1000, 3, 30, 7, 2.0)])
NEW = M.sigs([(1000, 0, 1, 1, 3.0), (5, 1, 2, 0, 4.0), (40, 0, 3, 2, 5.0)])
FN_MAP = np.array([8, 7, 9], dtype=np.int32)            # NEW's function 1 is the base's 7: k-mer 1000 names the same function


def test_empty_base_and_no_new_signatures():
    none = M.sigs([])
    U, c = _both(none, none)
    assert len(U) == 0 and c == dict.fromkeys(M.COUNTS, 0)
    U, c = _both(M.sigs([(EMPTY, 0, 0, 0, 0)] * 3), NEW)
    assert U["kmer"].tolist() == [5, 40, 1000] and c["added"] == 3 and c["base"] == 0 and c["merged"] == 3
    U, c = _both(BASE, none)                            # the export
    assert U.tolist() == [tuple(BASE[3]), tuple(BASE[1]), tuple(BASE[6])]
    assert c == dict(dict.fromkeys(M.COUNTS, 0), base=3, base_ignored=2, merged=3)


def test_each_policy_on_conflicts_with_the_same_and_another_function():
    mapped = M._mapped(NEW, FN_MAP, None)
    assert mapped["functionIndex"].tolist() == [7, 8, 9]
    U, c = _both(BASE, NEW, FN_MAP, None, "keep")
    assert U.tolist() == [tuple(mapped[1]), tuple(BASE[3]), tuple(BASE[1]), tuple(BASE[6])]
    assert c == {"base": 3, "base_ignored": 2, "added_in": 3, "added": 1, "conflicts": 2, "conflicts_same_function": 1, "replaced": 0,
                 "dropped": 0, "merged": 4}
    U, c = _both(BASE, NEW, FN_MAP, None, "replace")
    assert U.tolist() == [tuple(mapped[1]), tuple(BASE[3]), tuple(mapped[2]), tuple(mapped[0])]
    assert (c["replaced"], c["dropped"], c["merged"]) == (2, 0, 4)
    U, c = _both(BASE, NEW, FN_MAP, None, "drop")       # 40: functions 5 and 9, neither survives; 1000: 7 and 7, the base's
    assert U.tolist() == [tuple(mapped[1]), tuple(BASE[3]), tuple(BASE[6])]
    assert (c["replaced"], c["dropped"], c["merged"]) == (0, 1, 3)
    # without the map the raw indices are compared: 1000 names 7 and 1
    U, c = _both(BASE, NEW, None, None, "drop")
    assert U["kmer"].tolist() == [5, 7] and c["conflicts_same_function"] == 0 and c["dropped"] == 2


def test_all_conflicts():
    base = M.sigs([(v, 0, 0, v % 2, 1.0) for v in range(10)])
    new = M.sigs([(v, 1, 1, 0, 2.0) for v in range(9, -1, -1)])
    for policy, n, from_new in (("keep", 10, 0), ("replace", 10, 10), ("drop", 5, 0)):
        U, c = _both(base, new, None, None, policy)
        assert len(U) == n and int((U["otuIndex"] == 1).sum()) == from_new and c["conflicts"] == 10 and c["added"] == 0
        assert c["conflicts_same_function"] == 5


def test_every_error_and_its_precedence():
    bad = M.sigs([(3, 0, 0, 0, 1), (3, 5, 0, 7, 1), (-1, 0, 0, 0, 1), (M.MAX, 0, 0, 9, 1), (2, 0, 0, 0, 1), (2, 0, 0, 0, 1)])
    twice = M.sigs([(9, 0, 0, 0, 1), (4, 0, 0, 0, 1), (9, 0, 0, 0, 1), (4, 0, 0, 0, 1)])
    m2 = np.zeros(2, dtype=np.int32)
    e = _both(twice, bad, m2, m2)
    assert (e.kind, e.value) == ("kmer", 2)             # the k-mer range comes first, naming the smallest index
    ok_kmers = bad[[0, 1, 4, 5]]
    e = _both(twice, ok_kmers, m2, m2)
    assert (e.kind, e.value) == ("fn", 1)               # then the function map, before the OTU map
    e = _both(twice, ok_kmers, None, m2)
    assert (e.kind, e.value) == ("otu", 1)
    e = _both(twice, ok_kmers)
    assert (e.kind, e.value) == ("dup_new", 2)          # then a k-mer twice among the new ones: the smallest such k-mer
    e = _both(twice, ok_kmers[[0, 2]])
    assert (e.kind, e.value) == ("dup_base", 4)         # then a k-mer twice in the table
    assert e.message_parts() == ["duplicate k-mer 4 in the table"]
    e = _both(M.sigs([]), M.sigs([(1, 0, 0, 2, 1)]), np.zeros(2, dtype=np.int32))
    assert (e.kind, e.value) == ("fn", 0)               # n_fn itself is outside
    e = _both(M.sigs([]), M.sigs([(1, 0, 0, 0, 1)]), np.zeros(0, dtype=np.int32))
    assert (e.kind, e.value) == ("fn", 0)               # an empty map is a map


def test_the_bytes_are_moved_not_read():
    base = M.sigs([(3, -7, -9, 1, 0)])
    base.view(np.uint32).reshape(-1, 6)[0, 5] = 0x7FC00001
    new = M.sigs([(4, 0, 0, 0, 0)])
    new.view(np.uint32).reshape(-1, 6)[0, 5] = 0x80000000                # -0.0
    U, _ = _both(base, new)
    assert U.view(np.uint32).reshape(-1, 6)[:, 5].tolist() == [0x7FC00001, 0x80000000] and U[0]["otuIndex"] == -7


# ---- the union of the names ---------------------------------------------------------------------------------------------------

def test_name_union():
    base = b"0\talpha\n1\tbeta\n2\talpha\n3\tgamma\n"
    out, m = MT.unite_names(base, b"0\tbeta\n1\tdelta\n2\talpha\n3\tepsilon\n4\tdelta\n")
    assert out == base + b"4\tdelta\n5\tepsilon\n" and m.tolist() == [1, 4, 0, 5, 4] and m.dtype == np.int32
    out, m = MT.unite_names(base, None)
    assert out == base and m is None
    out, m = MT.unite_names(b"0\ta", b"0\tb\n")                          # no final newline in BASE: one is added before the new lines
    assert out == b"0\ta\n1\tb\n" and m.tolist() == [1]
    out, m = MT.unite_names(b"", b"0\tx\n")
    assert out == b"0\tx\n" and m.tolist() == [0]
    with pytest.raises(ValueError):
        MT.unite_names(b"0\ta\n2\tb\n", None)                            # loadIndexedArray: dense and in order


# ---- layouts ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cname,jname,py", [("kg_merge_params", "KgMergeParams", N.KgMergeParams), ("kg_merge_stats", "KgMergeStats", N.KgMergeStats)])
def test_jna_structures_match_the_c_layout(cname, jname, py):
    width = {"int32_t": "int", "uint32_t": "int", "int64_t": "long", "float": "float"}
    cf = H._c_struct(cname)
    jf, order = H._java_struct(jname)
    assert [n for n, _ in jf] == [n for n, _ in cf] == order
    assert [t for _, t in jf] == [width[t] for _, t in cf]
    assert [n for n, _ in py._fields_] == [n for n, _ in cf]
    assert list(M.COUNTS) == [n for n, t in cf if t == "int64_t"] or cname == "kg_merge_params"


def test_structures_match_gcc_layout(tmp_path):
    snames = [n for n, _ in N.KgMergeStats._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kmerguts_hip.h"\nint main(void){\n' +
                   'printf("%zu %zu %d %d %d\\n", sizeof(kg_merge_params), sizeof(kg_merge_stats), KG_MERGE_KEEP, KG_MERGE_REPLACE, KG_MERGE_DROP);\n' +
                   "".join('printf("%%zu\\n", offsetof(kg_merge_stats, %s));\n' % f for f in snames) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[:5] == [C.sizeof(N.KgMergeParams), C.sizeof(N.KgMergeStats), N.MERGE_KEEP, N.MERGE_REPLACE, N.MERGE_DROP]
    assert C.sizeof(N.KgMergeParams) == 8 and C.sizeof(N.KgMergeStats) == 9 * 8 + 4 * 4
    assert out[5:] == [getattr(N.KgMergeStats, f).offset for f in snames]
    assert N.MERGE_POLICIES == {"keep": 0, "replace": 1, "drop": 2}
    assert {"kg_table_merge_signatures", "kg_table_merge_signatures_device", "kg_sigset_merge_stats"} <= set(N.EXPORTS)


def test_the_documents_name_the_rule():
    for name in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, name)).read()
        assert "kg_table_merge_signatures" in text or "merge_tables" in text, name
    assert "9j" in open(os.path.join(ROOT, "DESIGN.md")).read()


# ---- the front end ------------------------------------------------------------------------------------------------------------

class ModelOps:
    """merge_tables.DeviceOps with the model in the place of the device calls"""

    def export(self, table_path):
        return M.merge_numpy(M.records_of_image(M.read_image(table_path))[1], M.sigs([]))[0]

    def merge(self, table_path, new, fn_map, otu_map, on_conflict):
        num_sigs, rec = M.records_of_image(M.read_image(table_path))
        U, c = M.merge_numpy(rec, M.sigs([]) if new is None else new, fn_map, otu_map, on_conflict)
        return U, c, num_sigs

    def place(self, u, num_sigs, path):
        image, placed = M.place(u, num_sigs)
        with (gzip.open if path.endswith(".gz") else open)(path, "wb") as f:
            f.write(image)
        return placed

    def records(self, u):
        return u

    def close(self, s):
        pass


def _data_dir(path, sig, num_sigs, fn_names, otu_names=None, gz=False):
    os.makedirs(path)
    image, placed = M.place(sig, num_sigs)
    assert placed == len(sig)
    with (gzip.open if gz else open)(os.path.join(path, "kmer.table.mem_map" + (".gz" if gz else "")), "wb") as f:
        f.write(image)
    with open(os.path.join(path, "function.index"), "wb") as f:
        f.write(b"".join(b"%d\t%s\n" % (i, n) for i, n in enumerate(fn_names)))
    if otu_names is not None:
        with open(os.path.join(path, "otu.index"), "wb") as f:
            f.write(b"".join(b"%d\t%s\n" % (i, n) for i, n in enumerate(otu_names)))
    return image


def test_front_end_files_and_summary_line(tmp_path, capsys):
    base_sig = M.sigs([(40, 1, 10, 0, 0.5), (7, 0, 20, 1, 1.0), (1000, 1, 30, 2, 2.0)])
    new_sig = M.sigs([(1000, 0, 1, 1, 3.0), (5, 1, 2, 0, 4.0), (40, 0, 3, 2, 5.0)])
    base, new, out = str(tmp_path / "base"), str(tmp_path / "new"), str(tmp_path / "out")
    base_image = _data_dir(base, base_sig, 11, [b"kinase", b"ligase", b"kinase", b"lyase"], [b"genome A", b"genome B"], gz=True)
    _data_dir(new, new_sig, 13, [b"permease", b"lyase", b"ligase"], [b"genome C", b"genome A"])
    r = MT.merge_tables(base, out, new, on_conflict="drop", sigs_out=str(tmp_path / "u.txt.gz"), ops=ModelOps())
    fn_map, otu_map = np.array([4, 3, 1], dtype=np.int32), np.array([2, 0], dtype=np.int32)
    U, c = M.merge_numpy(M.records_of_image(base_image)[1], new_sig, fn_map, otu_map, "drop")
    assert U["kmer"].tolist() == [5, 7] and c["dropped"] == 2       # 1000: lyase (3) against kinase (2); 40: ligase (1) against kinase (0)
    assert open(os.path.join(out, "function.index"), "rb").read() == b"0\tkinase\n1\tligase\n2\tkinase\n3\tlyase\n4\tpermease\n"
    assert open(os.path.join(out, "otu.index"), "rb").read() == b"0\tgenome A\n1\tgenome B\n2\tgenome C\n"
    assert open(os.path.join(out, "kmer.table.mem_map"), "rb").read() == M.place(U, 11)[0]        # max(11, next_prime(4))
    assert parse_signatures(gzip.open(str(tmp_path / "u.txt.gz")).read()).tobytes() == U.tobytes()
    assert MT.summary_line(r) == ("Base: 3 (ignored 0), new: 3, added: 1, conflicts: 2 (same function: 0), replaced: 0, dropped: 2, "
                                  "merged: 2, slots: 11, placed: 2, dropped at the end: 0")
    # a dump of BASE: --sigs without --add, no table placed; fed to make_table's parser it gives the base's signatures
    r = MT.merge_tables(base, sigs_out=str(tmp_path / "dump.txt"), ops=ModelOps())
    dump = open(str(tmp_path / "dump.txt")).read()
    assert dump == signature_text(np.sort(base_sig, order="kmer")) and MT.summary_line(r).endswith("dropped: 0, merged: 3")
    assert M.place(parse_signatures(dump.encode()), 11)[0] == base_image
    # replace, a chosen size, gzip
    out2 = str(tmp_path / "out2")
    r = MT.merge_tables(base, out2, new, num_sigs=5, gz=True, on_conflict="replace", ops=ModelOps())
    U, c = M.merge_numpy(M.records_of_image(base_image)[1], new_sig, fn_map, otu_map, "replace")
    image, placed = M.place(U, 5)
    assert gzip.open(os.path.join(out2, "kmer.table.mem_map.gz")).read() == image and (r["slots"], r["placed"], r["replaced"]) == (5, placed, 2)
    # refusals
    with pytest.raises(FileExistsError):                # OUTDIR holds the .gz the readers would take
        MT.merge_tables(base, out2, new, ops=ModelOps())
    for bad_out in (base, new, os.path.join(str(tmp_path), "x", "..", "base")):
        with pytest.raises(ValueError):
            MT.merge_tables(base, bad_out, new, ops=ModelOps())
    with pytest.raises(ValueError):
        MT.merge_tables(base, None, new, ops=ModelOps())
    assert MT.main(["-D", base, "--add", new]) == 1 and "at least one of -o and --sigs" in capsys.readouterr().err


def test_front_end_without_an_otu_index_in_base(tmp_path, capsys):
    base, new, out = str(tmp_path / "base"), str(tmp_path / "new"), str(tmp_path / "out")
    _data_dir(base, M.sigs([(40, 1, 10, 0, 0.5)]), 3, [b"kinase"])
    _data_dir(new, M.sigs([(5, 1, 2, 0, 4.0)]), 3, [b"kinase"], [b"genome C", b"genome A"])
    r = MT.merge_tables(base, out, new, ops=ModelOps())
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and err.startswith("Warning: ") and "otu.index" in err
    assert sorted(os.listdir(out)) == ["function.index", "kmer.table.mem_map"] and r["merged"] == 2
    U = M.records_of_image(open(os.path.join(out, "kmer.table.mem_map"), "rb").read())[1]
    assert sorted(U[U["kmer"] < M.MAX].tolist()) == [(5, 1, 2, 0, 4.0), (40, 1, 10, 0, 0.5)]       # OTU index 1 kept as it is
    assert open(os.path.join(out, "function.index"), "rb").read() == b"0\tkinase\n"


def test_front_end_prints_a_library_error_with_the_letters(capsys, monkeypatch, tmp_path):
    base = str(tmp_path / "base")
    _data_dir(base, M.sigs([(40, 1, 10, 0, 0.5)]), 3, [b"kinase"])

    class Failing(ModelOps):
        def merge(self, *a):
            raise N.KmerGutsNativeError(-1, "duplicate k-mer 21 in the table (the smallest k-mer that occurs more than once)")

    monkeypatch.setattr(MT, "DeviceOps", lambda device=0: Failing())
    assert MT.main(["-D", base, "--sigs", str(tmp_path / "x.txt")]) == 1
    assert "duplicate k-mer AAAAAACC (21) in the table" in capsys.readouterr().err
