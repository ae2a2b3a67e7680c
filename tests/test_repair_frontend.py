"""call_regions --repair on the CPU, the device calls replaced by the models (the oracle's DNA scan, regions_model, orfs_model,
repair_model and the later stages' models): the writers, the summary, the options; the bytes without --repair against digests
recorded from the commit before the option existed; and the finding the option is for, on the planted contigs."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import coding_model as K  # noqa: E402
import free_orfs_model as F  # noqa: E402
import orfs_model as O  # noqa: E402
import regions_model as R  # noqa: E402
import repair_model as M  # noqa: E402
import select_model as S  # noqa: E402
import starts_model as SM  # noqa: E402
import test_coding_host as TH  # noqa: E402
import test_orfs_host as HO  # noqa: E402
import test_starts_host as SH  # noqa: E402


class _ModelScan(SH._ModelScan):
    """test_starts_host's stand-in for a ScanResult with repair= added, as hotpath has it: between the ORFs and the free ORFs."""

    def orfs(self, seq, offsets, merge_gap=600, min_score=0, min_len=0, start_codons=7, only_kept=True, device_ptr=None,
             free_min_res=None, coding=None, min_coding=0, min_train_pairs=100000, starts=None, start_min_res=100, start_rounds=4,
             min_train_starts=200, repair=False, repair_min_count=0, max_junctions=4):
        if not repair:
            return SH._ModelScan.orfs(self, seq, offsets, merge_gap, min_score, min_len, start_codons, only_kept, device_ptr, free_min_res,
                                      coding, min_coding, min_train_pairs, starts, start_min_res, start_rounds, min_train_starts)
        regs, start = self.regions(offsets, merge_gap, min_score, min_len)
        o, ps, res = O.orfs(regs, self.seq, self.off, start_codons, only_kept)
        o, ps, res, self.junctions, self.junction_start, self.repair_stats = M.repair(regs, o, ps, res, self.calls, self.seq, self.off,
                                                                                      start_codons, repair_min_count, max_junctions)
        got = (o, ps, res)
        if free_min_res is not None:
            got = F.concat(got, F.free_orfs(self.seq, self.off, free_min_res, start_codons))
        if coding is not None:
            recs, self.coding_scores, self.coding_stats, self.coding_model = K.coding(got[0], self.seq, self.off, None if coding is True else coding,
                                                                                      min_coding, min_train_pairs)
            got = (recs,) + tuple(got[1:])
        if starts is not None and starts is not False:
            T = K.table(*self.coding_model) if coding is True else coding
            out = SM.starts(got[0], self.seq, self.off, T, None if starts is True else starts, SM.region_limits(got[0], regs, self.off),
                            start_min_res, start_codons, start_rounds, min_train_starts, prot_start=got[1], residues=got[2], scores=self.coding_scores)
            self.start_shifts, self.start_stats, self.start_model = out["shifts"], out["stats"], out["model"]
            self.coding_scores = out["scores"]
            got = (out["orfs"], out["prot_start"], out["residues"])
        return (regs, start) + tuple(got)

    def select(self, offsets, seq=None, merge_gap=600, min_score=0, min_len=0, orfs=False, start_codons=7, only_kept=True,
               device_ptr=None, max_overlap=60, max_overlap_pct=50, **kw):
        assert orfs
        got = self.orfs(seq, offsets, merge_gap, min_score, min_len, start_codons, only_kept, None, **kw)
        return got + (S.select_fast(S.of_records(got[2]), max_overlap, max_overlap_pct),)


def _front_end(oracle, tmp_path, monkeypatch):
    ids, fnames, dna, off, d, q, made = TH._front_end(oracle, tmp_path, monkeypatch)
    from kmergutsjava_amd import kmer_guts_java as KGJ
    img = TH._WORK["w"][0]

    class _Table:
        def scan(self, batch, boff, params):
            ora = oracle.run(img, np.frombuffer(batch, dtype=np.uint8), boff, lookup_mode=1, min_hits=params.min_hits)
            made.append(_ModelScan(ora["calls"], batch, np.asarray(boff, dtype=np.int64)))
            return made[-1]

    monkeypatch.setattr(KGJ, "_resident_table", lambda path, device: _Table())
    return ids, fnames, dna, off, d, q, made


KW = dict(min_hits=4, merge_gap=300, min_score=12, min_len=100)


def test_call_regions_with_repair_against_the_models(oracle, tmp_path, monkeypatch):
    from kmergutsjava_amd import call_regions as CR
    ids, fnames, dna, off, d, q, made = _front_end(oracle, tmp_path, monkeypatch)

    def run(tag, **more):
        line = CR.call_regions(d, q, str(tmp_path / (tag + ".tsv")), orfs_out=str(tmp_path / (tag + ".orfs")), faa_out=str(tmp_path / (tag + ".faa")),
                               shifts_out=str(tmp_path / (tag + ".shifts")) if more.get("repair") else None, **KW, **more)
        return line, [(tmp_path / (tag + ext)).read_bytes() for ext in (".tsv", ".orfs", ".faa")]

    line, files = run("rep", repair=True)
    regs, start, orfs, ps, res = made[-1].orfs(dna, off, 300, 12, 100, repair=True)
    junc, st = made[-1].junctions, made[-1].repair_stats
    rep = (orfs["flags"] & M.REPAIRED) != 0
    assert st["repaired"] == rep.sum() >= 20 and st["candidates"] >= st["repaired"]
    assert line == CR.summary_of(regs, start) + CR.orf_summary(orfs) + ", repaired: %d, unrepaired: %d" % (st["repaired"], st["candidates"] - st["repaired"])
    assert files[1] == CR.format_orfs(ids, regs, orfs, fnames) and files[2] == CR.format_faa(ids, regs, orfs, ps, res, fnames)
    # every repaired ORF's line has the flag word, its new frame, extent and length; no other line has it
    rows = [ln.split(b"\t") for ln in files[1].splitlines()]
    assert sum(b"repaired" in f[9].split(b",") for f in rows) == rep.sum() == files[1].count(b"repaired")
    for f in rows:
        if b"repaired" in f[9].split(b","):
            assert {b"interrupted", b"multi-frame"} <= set(f[9].split(b","))
    # the shifts file: one line per junction, the ORF's extent in front
    shifts = (tmp_path / "rep.shifts").read_bytes()
    assert shifts == CR.format_shifts(ids, regs, orfs, fnames, junc) and shifts.count(b"\n") == len(junc) == st["junctions"] > 0
    j, o = junc[0], orfs[junc[0]["orf"]]
    assert shifts.splitlines()[0] == b"%s\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d" % (ids[o["seq"]], o["left"] + 1, o["right"] + 1, b"-" if o["strand"] else b"+",
                                                                             fnames[o["fI"]], j["pos"] + 1, j["from_frame"], j["to_frame"], j["res"] + 1,
                                                                             j["gap"])
    # the protein file holds the chain, not the read-through
    i = int(np.flatnonzero(rep)[0])
    head = b">%s_%d_%d_%s " % (ids[int(orfs[i]["seq"])], orfs[i]["left"] + 1, orfs[i]["right"] + 1, b"-" if orfs[i]["strand"] else b"+")
    assert files[2].split(head)[1].split(b"\n", 1)[1].replace(b"\n", b"").startswith(res[ps[i]:ps[i + 1]].tobytes())
    # behind it: free ORFs, coding, starts and the selection see the new extents; repaired records are not moved
    more = dict(free_min_res=100, coding=True, min_train=1000, starts=True, min_train_starts=50)
    line_s, files_s = run("sel", repair=True, select=True, **more)
    skw = dict(free_min_res=100, coding=True, min_train_pairs=1000, starts=True, min_train_starts=50, repair=True)
    full = made[-1].select(off, dna, 300, 12, 100, True, 7, True, **skw)
    nr = len(regs)
    assert full[2][:nr][rep].tobytes() == orfs[rep].tobytes() and not made[-1].start_shifts[:nr][rep].any()
    assert not any(K.is_training(o) for o in orfs[rep]) and not any(SM.is_movable(o) for o in orfs[rep])
    assert ", repaired: %d, unrepaired: %d, selected: " % (st["repaired"], st["candidates"] - st["repaired"]) in line_s
    assert full[5].tobytes() == S.select_fast(S.of_records(full[2])).tobytes() and (full[5]["state"][:nr][rep] == 1).any()
    assert (tmp_path / "sel.shifts").read_bytes() == CR.format_shifts(ids, regs, full[2][:nr], fnames, junc, sel=full[5][:nr])
    # --all writes every junction
    run("all", repair=True, select=True, write_all=True, **more)
    assert (tmp_path / "all.shifts").read_bytes().count(b"\n") == len(junc)
    # parameters reach the step
    line_1, _ = run("one", repair=True, repair_min_count=10 ** 6)
    assert line_1.endswith(", repaired: 0, unrepaired: %d" % st["candidates"]) and (tmp_path / "one.shifts").read_bytes() == b""


def same_as_recorded(key: str, line: str, files) -> None:
    """tests/golden/call_regions_planted_before_repair.json: the summary line and sha256, bytes and lines of the three files the
    front end wrote with --coding --starts for the planted contigs before it knew --repair (recorded from that commit's writers)."""
    want = json.load(open(os.path.join(HERE, "golden", "call_regions_planted_before_repair.json")))["runs"][key]
    assert line == want["summary"], (key, line, want["summary"])
    for name, data in zip(("tsv", "orfs", "faa"), files):
        got = {"sha256": hashlib.sha256(data).hexdigest(), "bytes": len(data), "lines": data.count(b"\n")}
        assert got == want[name], (key, name, got, want[name])


@pytest.mark.parametrize("write_all", [False, True])
@pytest.mark.parametrize("select", [False, True])
def test_call_regions_without_repair_writes_the_recorded_bytes(oracle, tmp_path, monkeypatch, write_all, select):
    from kmergutsjava_amd import call_regions as CR
    ids, fnames, dna, off, d, q, made = _front_end(oracle, tmp_path, monkeypatch)
    line = CR.call_regions(d, q, str(tmp_path / "p.tsv"), orfs_out=str(tmp_path / "p.orfs"), faa_out=str(tmp_path / "p.faa"), free_min_res=100,
                           coding=True, min_train=1000, starts=True, min_train_starts=50, write_all=write_all, select=select, **KW)
    assert "repaired" not in line
    same_as_recorded("starts_" + ("all" if write_all else "written") + ("_select" if select else ""), line,
                     [(tmp_path / ("p" + ext)).read_bytes() for ext in (".tsv", ".orfs", ".faa")])


def test_repair_options_need_their_partners():
    from kmergutsjava_amd import call_regions as CR
    with pytest.raises(ValueError):
        CR.call_regions("nowhere", "none.fna", "out.tsv", repair=True)
    with pytest.raises(ValueError):
        CR.call_regions("nowhere", "none.fna", "out.tsv", orfs_out="x", shifts_out="s")
    for argv in (["--repair"], ["--orfs", "x", "--shifts", "s"], ["--orfs", "x", "--repair-min-count", "2"], ["--orfs", "x", "--max-junctions", "2"]):
        with pytest.raises(SystemExit):
            CR.main(["-D", "d", "-q", "q", "-o", "o"] + argv)
    assert CR.repair_summary(3, 5) == ", repaired: 3, unrepaired: 2"
    assert (128, b"repaired") in CR.FLAG_WORDS


def _holds_both_ends(text: str, prot: str) -> bool:
    return prot[:20] in text and prot[-20:] in text


def test_the_finding_on_the_planted_contigs(oracle):
    """Every third planted gene has one base deleted in its middle.  Counted: the shifted genes whose written protein (of a region
    of their strand and function that overlaps them) holds both the planted protein's residues 1..20 and its last 20.
    Measured with this model: 0 of 40 without the repair, 35 with it; 35 regions repaired, all of them planted shifted genes;
    J minus the deletion's position, on the gene's strand, lies between -62 and +21 nucleotides, median -2."""
    img, dna, off, genes = HO.planted_orf_contigs()
    ora = oracle.run(img, np.frombuffer(dna, dtype=np.uint8), off, lookup_mode=1)
    regs, start = R.regions(ora["calls"], off)
    o, ps, res = O.orfs(regs, dna, off)
    new = M.repair(regs, o, ps, res, ora["calls"], dna, off)

    def count(orfs, pstart, residues):
        n, hit_regions = 0, set()
        text = residues.tobytes().decode()
        for c, left, right, strand, f, shifted, prot in genes:
            if not shifted:
                continue
            sl = slice(int(start[c]), int(start[c + 1]))
            hit = np.flatnonzero((regs[sl]["strand"] == strand) & (regs[sl]["fI"] == f) & (regs[sl]["left"] <= right) & (regs[sl]["right"] >= left)) + sl.start
            good = [k for k in hit if _holds_both_ends(text[pstart[k]:pstart[k + 1]], prot)]
            n += bool(good)
            hit_regions |= set(int(k) for k in hit)
        return n, hit_regions

    before, planted = count(o, ps, res)
    after, _ = count(new[0], new[1], new[2])
    rep = np.flatnonzero((new[0]["flags"] & M.REPAIRED) != 0)
    # J - deletion, on the gene's strand
    dist = []
    for c, left, right, strand, f, shifted, prot in genes:
        if not shifted:
            continue
        mid = (right - left + 2) // 2                   # index in the planted gene's own DNA of the deleted base
        cut = left + mid if not strand else right - mid       # where the base behind the deleted one now stands
        for j in new[3]:
            r = new[0][j["orf"]]
            if r["seq"] == c and r["strand"] == strand and r["fI"] == f and r["left"] <= right and r["right"] >= left:
                dist.append(int(j["pos"] - cut) if not strand else int(cut - j["pos"]))
    print("shifted genes %d; both ends in the written protein: %d without the repair, %d with it; repaired regions %d, of which planted %d; "
          "J - deletion: min %d, median %d, max %d" % (sum(g[5] for g in genes), before, after, len(rep), len(set(rep.tolist()) & planted),
                                                      min(dist), int(np.median(dist)), max(dist)))
    assert after > before
    # every unshifted gene's record is unchanged: no repaired region overlaps one on its strand with its function
    for c, left, right, strand, f, shifted, prot in genes:
        if shifted:
            continue
        sl = slice(int(start[c]), int(start[c + 1]))
        hit = np.flatnonzero((regs[sl]["strand"] == strand) & (regs[sl]["fI"] == f) & (regs[sl]["left"] <= right) & (regs[sl]["right"] >= left)) + sl.start
        assert new[0][hit].tobytes() == o[hit].tobytes(), (c, left, right)
        for k in hit:
            assert new[2][new[1][k]:new[1][k + 1]].tobytes() == res[ps[k]:ps[k + 1]].tobytes()
